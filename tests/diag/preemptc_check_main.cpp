// preemptc_check_main.cpp -- csrc/ksched_preemptc.h's host side on its own, for a CPU sanitizer run of
// ksched_load_bound_constrained's and ksched_preempt_constrained's checks: every KSCHED_E_INVALID and KSCHED_E_STATE
// case in include/ksched.h's order, the packing of the table's two extra columns and of the pods' constraint words (no
// device call, no library):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ik8s-scheduler_amd/csrc
//       tests/diag/preemptc_check_main.cpp -o preemptc_check; ./preemptc_check
// Every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ksched_preemptc.h"

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

// ---- the table ---------------------------------------------------------------------------------------------------------
struct Table {
    int64_t nb = 0, n_local = 3;
    std::vector<int32_t> node, prio;
    std::vector<int64_t> cpu, mem, ext;
    std::vector<uint64_t> mask;
    int32_t n_ext = 0;
};

static const char *check(const Table &t) {
    Exact<int32_t> node(t.node), prio(t.prio);
    Exact<int64_t> cpu(t.cpu), mem(t.mem), ext(t.ext);
    Exact<uint64_t> mask(t.mask);
    return pc_check_bound(PcBound{t.nb, node.p, cpu.p, mem.p, prio.p, t.n_ext, ext.p, mask.p}, t.n_local);
}

// four pods on three nodes, two columns
static Table table() {
    Table t;
    t.nb = 4;
    t.node = {2, 0, 0, 1}; t.prio = {5, 6, 7, 8};
    t.cpu = {10, 20, 30, 40}; t.mem = {1, 2, 3, 4};
    t.n_ext = 2; t.ext = {1, 0, 2, 0, 0, 3, 0, 4};
    t.mask = {1, 0, 6, (uint64_t)1 << 63};
    return t;
}

// ---- the call ----------------------------------------------------------------------------------------------------------
struct Call {
    int64_t m = 0;
    std::vector<int64_t> rc, rm, rp;
    std::vector<uint64_t> sel;
    std::vector<int32_t> prio, group;
    std::vector<uint8_t> enforce;
    std::vector<int64_t> req;
    int32_t vcap = 4;
    PcState st{true, false, 1, true, 2, 3, 2, 2};  // nodes, a bound table with two columns and masks {0, 1}, S = 2, R = 2
};

static PcPacked packed;
static const char *why;

static int run(const Call &c) {
    Exact<int64_t> rc(c.rc), rm(c.rm), rp(c.rp), req(c.req);
    Exact<int32_t> prio(c.prio), group(c.group);
    Exact<uint8_t> enf(c.enforce);
    Exact<uint64_t> sel(c.sel);
    packed = PcPacked{};
    return pc_check_pack(PcCall{c.m, rc.p, rm.p, rp.p, sel.p, prio.p, group.p, enf.p, req.p, c.vcap}, c.st, &packed, &why);
}

// three pods, both constraints on
static Call both_on() {
    Call c;
    c.m = 3;
    c.rc = {100, 200, 300}; c.rm = {1, 2, 3}; c.rp = {1, 1, 2}; c.prio = {10, 20, 30};
    c.group = {0, 1, -1}; c.enforce = {1, 0, 1};
    c.req = {1, 0, 2, 0, 0, 3};
    return c;
}

int main() {
    {   // ksched_load_bound_constrained: ksched_load_bound's cases, then the columns'
        expect(check(table()) == nullptr, "a valid table");
        Table t;
        expect(check(t) == nullptr, "the empty table");
        t = table(); t.nb = -1;
        expect(check(t) != nullptr, "nb < 0");
        t = table(); t.nb = 0x7fffffff;
        expect(check(t) != nullptr, "nb = 2^31 - 1: refused before any array is read");
        t = table(); t.prio.clear();
        expect(check(t) != nullptr, "a NULL prio");
        t = table(); t.n_ext = -1;
        expect(check(t) != nullptr, "n_ext < 0");
        t = table(); t.n_ext = KSCHED_EXT_MAX + 1;
        expect(check(t) != nullptr, "n_ext above KSCHED_EXT_MAX: refused before bound_ext is read");
        t = table(); t.ext.clear();
        expect(check(t) != nullptr, "a NULL bound_ext with n_ext > 0");
        t = table(); t.n_ext = 0;
        expect(check(t) != nullptr, "bound_ext given with n_ext == 0");
        t = table(); t.n_ext = 0; t.ext.clear();
        expect(check(t) == nullptr, "masks alone");
        t = table(); t.mask.clear();
        expect(check(t) == nullptr, "columns alone");
        t = table(); t.node[2] = 3;
        expect(check(t) != nullptr, "a node index of n_local");
        t = table(); t.node[0] = -1;
        expect(check(t) != nullptr, "a negative node index");
        t = table(); t.n_local = 0;
        expect(check(t) != nullptr, "pods and no nodes");
        t = table(); t.ext[7] = -1;
        expect(check(t) != nullptr, "a negative amount in the last cell");
        {   // one node at the segment bound, then one above
            Table f;
            f.nb = KSCHED_BOUND_MAX_PER_NODE;
            f.node.assign((size_t)f.nb, 1); f.prio.assign((size_t)f.nb, 0);
            f.cpu.assign((size_t)f.nb, 1); f.mem.assign((size_t)f.nb, 0);
            expect(check(f) == nullptr, "KSCHED_BOUND_MAX_PER_NODE pods on one node");
            f.nb += 1; f.node.push_back(1); f.prio.push_back(0); f.cpu.push_back(1); f.mem.push_back(0);
            expect(check(f) != nullptr, "one more");
        }
    }
    {   // the packing: entry e holds its table pod's amounts and mask, padding nothing
        const Table t = table();
        const std::vector<int32_t> tidx = {1, -1, 3, 2, -1, 0, -1, -1};
        std::vector<int64_t> ext;
        std::vector<uint64_t> mask;
        uint64_t mask_or = 0;
        pc_pack_columns(tidx, PcBound{t.nb, t.node.data(), t.cpu.data(), t.mem.data(), t.prio.data(), t.n_ext, t.ext.data(), t.mask.data()},
                        &ext, &mask, &mask_or);
        expect(ext == std::vector<int64_t>({0, 0, 0, 2, 0, 1, 0, 0, 3, 0, 4, 0, 0, 0, 0, 0}), "ext columns, slot-major beside tidx");
        expect(mask == std::vector<uint64_t>({0, 0, (uint64_t)1 << 63, 6, 0, 1, 0, 0}), "masks");
        expect(mask_or == (((uint64_t)1 << 63) | 7), "every mask ORed");
        pc_pack_columns(tidx, PcBound{t.nb, t.node.data(), t.cpu.data(), t.mem.data(), t.prio.data(), 0, nullptr, nullptr}, &ext, &mask, &mask_or);
        expect(ext.empty() && mask == std::vector<uint64_t>(8, 0) && mask_or == 0, "ksched_load_bound's table: no column, zero masks");
    }
    {   // the pods' words: the group only where the pod enforces, requests pod-major
        expect(run(both_on()) == KSCHED_OK && packed.spread && packed.ext, "both on");
        expect(packed.sg == std::vector<int32_t>({0, -1, -1}), "a pod that only counts enforces nothing");
        expect(packed.er == std::vector<int64_t>({1, 0, 0, 0, 0, 0, 0, 0, 2, 3, 0, 0}), "extended requests, pod-major");
        Call c;
        c.m = 2; c.rc = {1, 2}; c.rm = {3, 4}; c.rp = {1, 1}; c.prio = {0, 0};
        c.st = PcState{true, false, 1, true, 0, 0, 0, 0};
        expect(run(c) == KSCHED_OK && !packed.spread && !packed.ext, "both off: no table is needed");
        expect(packed.sg == std::vector<int32_t>({-1, -1}) && packed.er == std::vector<int64_t>(8, 0), "off: no words");
        c.m = 0; c.rc.clear(); c.rm.clear(); c.rp.clear(); c.prio.clear();
        expect(run(c) == KSCHED_OK && packed.sg.empty(), "no pods");
        c = both_on(); c.enforce.clear();
        expect(run(c) == KSCHED_OK && packed.sg == std::vector<int32_t>({0, 1, -1}), "a NULL spread_enforce: every pod enforces");
    }
    {   // KSCHED_E_INVALID, in the header's order -- each one also before every state error (st: nothing loaded at all)
        const PcState nothing{false, false, 1, false, 0, 0, 0, 0};
        Call c = both_on(); c.vcap = 0;
        expect(run(c) == KSCHED_E_INVALID, "vcap 0");
        c.st = nothing;
        expect(run(c) == KSCHED_E_INVALID, "vcap 0 before load_nodes");
        c = both_on(); c.vcap = KSCHED_BOUND_MAX_PER_NODE + 1;
        expect(run(c) == KSCHED_E_INVALID, "vcap above KSCHED_BOUND_MAX_PER_NODE");
        c = both_on(); c.m = -1;
        expect(run(c) == KSCHED_E_INVALID, "m < 0");
        c = both_on(); c.m = (int64_t)1 << 30; c.st = nothing;
        expect(run(c) == KSCHED_E_INVALID, "m = 2^30: refused before any array is read");
        c = both_on(); c.rm.clear();
        expect(run(c) == KSCHED_E_INVALID, "a NULL request array");
        c = both_on(); c.prio.clear(); c.st = nothing;
        expect(run(c) == KSCHED_E_INVALID, "a NULL prio");
        c = both_on(); c.st.use_labels = true;
        expect(run(c) == KSCHED_E_INVALID, "use_labels without selectors");
        c.sel = {1, 2, 4};
        expect(run(c) == KSCHED_OK, "selectors");
        c = both_on(); c.st.nranks = 2;
        expect(run(c) == KSCHED_E_INVALID, "opts.nranks > 1");
        c.st = nothing; c.st.nranks = 2;
        expect(run(c) == KSCHED_E_INVALID, "opts.nranks > 1 before load_nodes");
        c = both_on(); c.group = {0, 2, -1};
        expect(run(c) == KSCHED_E_INVALID, "a spread group of S");
        c.st.bound_valid = false;
        expect(run(c) == KSCHED_E_INVALID, "a spread group of S, and no bound table");
        c = both_on(); c.group = {0, -2, -1};
        expect(run(c) == KSCHED_E_INVALID, "a spread group below -1");
        c.st = nothing;
        expect(run(c) == KSCHED_E_INVALID, "a spread group below -1 without a table");
        c = both_on(); c.req = {1, 0, 2, 0, -1, 3};
        expect(run(c) == KSCHED_E_INVALID, "a negative extended-resource request");
        c.st.bound_R = 1;
        expect(run(c) == KSCHED_E_INVALID, "a negative request, and a table of another n_ext");
    }
    {   // KSCHED_E_STATE, in the header's order
        Call c = both_on(); c.st.nodes_loaded = false; c.st.bound_valid = false;
        expect(run(c) == KSCHED_E_STATE, "before load_nodes");
        c = both_on(); c.st.bound_valid = false;
        expect(run(c) == KSCHED_E_STATE, "no bound-pod table");
        c = both_on(); c.st.spread_S = 0; c.group = {7, 7, 7};
        expect(run(c) == KSCHED_E_STATE, "spread on without a table (no S to check the groups against)");
        c = both_on(); c.st.ext_R = 0; c.req.clear(); c.req = {1};  // (an array of unknown length is never read)
        expect(run(c) == KSCHED_E_STATE, "ext on without a table");
        c = both_on(); c.st.bound_R = 0;
        expect(run(c) == KSCHED_E_STATE, "req_ext given and ksched_load_bound's table");
        c = both_on(); c.st.bound_R = 3;
        expect(run(c) == KSCHED_E_STATE, "req_ext given and a table of another n_ext");
        c.req.clear();
        expect(run(c) == KSCHED_OK, "ext off: the table's n_ext does not matter");
        c = both_on(); c.st.bound_mask_or = 4;
        expect(run(c) == KSCHED_E_STATE, "a mask bit at S");
        c.group.clear(); c.enforce.clear();
        expect(run(c) == KSCHED_OK, "spread off: the masks do not matter");
        c = both_on(); c.st.spread_S = 64; c.st.bound_mask_or = ~(uint64_t)0;
        expect(run(c) == KSCHED_OK, "S = 64: every bit names a group");
        c = both_on(); c.st.bound_mask_or = (uint64_t)1 << 63;
        expect(run(c) == KSCHED_E_STATE, "bit 63 with S = 2");
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("preemptc_check: all checks passed\n");
    return 0;
}
