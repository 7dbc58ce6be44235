// affinity_check_main.cpp -- csrc/ksched_affinity.h on its own, for a CPU sanitizer run of the table check, the zone /
// any derivation and the per-pod packing of ksched_load_affinity / ksched_schedule_affinity (no device call, no library):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ik8s-scheduler_amd/csrc
//       tests/diag/affinity_check_main.cpp -o affinity_check; ./affinity_check
// Every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ksched_affinity.h"

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

static const char *table(int64_t n, int32_t D, const std::vector<int32_t> &dom) {
    Exact<int32_t> d(dom);
    return aff_check_table(n, D, d.p);
}

int main() {
    // ---- the table check: every KSCHED_E_INVALID case of ksched_load_affinity, and the valid edges beside it
    expect(table(4, 2, {0, 1, 0, -1}) == nullptr, "the worked example's domains");
    expect(table(4, -1, {-1, -1, -1, -1}) != nullptr, "D -1");
    expect(table(4, INT32_MIN, {-1, -1, -1, -1}) != nullptr, "D INT32_MIN");
    expect(table(4, KSCHED_SPREAD_MAX_DOMAINS + 1, {0, 1, 2, 3}) != nullptr, "D above the cap");
    expect(table(4, INT32_MAX, {0, 1, 2, 3}) != nullptr, "D INT32_MAX");
    expect(table(4, 2, {0, 2, 1, -1}) != nullptr, "a node domain of D");
    expect(table(4, 2, {0, 1, -2, -1}) != nullptr, "a node domain of -2");
    expect(table(4, 2, {0, 1, INT32_MAX, -1}) != nullptr, "a node domain of INT32_MAX");
    expect(table(4, 2, {0, 1, INT32_MIN, -1}) != nullptr, "a node domain of INT32_MIN");
    expect(table(4, 3, {0, 1, 0, -1}) != nullptr, "the last domain carried by no node");
    expect(table(4, 3, {0, 2, 0, -1}) != nullptr, "a domain below the largest carried by no node");
    expect(table(4, 2, {}) != nullptr, "node_domain NULL with D > 0 and n > 0");
    expect(table(0, 2, {}) == nullptr, "node_domain NULL with D > 0 and no node: nothing to read");
    expect(table(0, 1, {}) == nullptr, "no node at all");
    expect(table(4, 0, {}) == nullptr, "D 0 with node_domain NULL: host scope only");
    expect(table(4, 0, {-1, -1, -1, -1}) == nullptr, "D 0 with every node -1");
    expect(table(4, 0, {-1, 0, -1, -1}) != nullptr, "D 0 with a node in domain 0");
    {
        std::vector<int32_t> dom(1100);
        for (int j = 0; j < 1100; ++j) dom[j] = j % KSCHED_SPREAD_MAX_DOMAINS;
        expect(table(1100, KSCHED_SPREAD_MAX_DOMAINS, dom) == nullptr, "D at the cap");
        dom[1023] = 0;
        expect(table(1100, KSCHED_SPREAD_MAX_DOMAINS, dom) != nullptr, "D at the cap, the last id carried by no node");
    }
    // ---- the derivation: zone words per domain, side by side, and the any words; null masks are zeros
    {
        const Exact<int32_t> dom({0, 1, 0, -1});
        const Exact<uint64_t> mem({1, 2, 4, 8}), az({16, 32, 64, 128});
        AffDerived d;
        aff_derive(4, 2, dom.p, mem.p, az.p, &d);
        expect(d.zone.size() == 4 && d.zone[0] == 5 && d.zone[1] == 80 && d.zone[2] == 2 && d.zone[3] == 32, "zone words");
        expect(d.any_host == 15 && d.any_zone == 7, "any words: the node without the key counts for the host scope only");
        aff_derive(4, 2, dom.p, nullptr, nullptr, &d);
        expect(d.zone == std::vector<uint64_t>(4, 0) && d.any_host == 0 && d.any_zone == 0, "null masks");
        aff_derive(4, 2, dom.p, mem.p, nullptr, &d);
        expect(d.zone[0] == 5 && d.zone[1] == 0 && d.any_host == 15, "a null node_anti_zone");
        aff_derive(4, 0, nullptr, mem.p, az.p, &d);
        expect(d.zone.empty() && d.any_host == 15 && d.any_zone == 0, "no zone key");
        aff_derive(0, 0, nullptr, nullptr, nullptr, &d);
        expect(d.zone.empty() && d.any_host == 0, "no node");
        const Exact<uint64_t> top({(uint64_t)1 << 63, 0, 0, 0});
        aff_derive(4, 2, dom.p, top.p, top.p, &d);
        expect(d.zone[0] == (uint64_t)1 << 63 && d.zone[1] == (uint64_t)1 << 63 && d.any_zone == (uint64_t)1 << 63, "group 63");
    }
    // ---- the packing: every KSCHED_E_INVALID case of ksched_schedule_affinity, then the words
    std::vector<int32_t> words;
    std::vector<uint64_t> pods;
    auto pack = [&](int64_t p, const std::vector<uint64_t> &m, const std::vector<uint64_t> &ah, const std::vector<uint64_t> &az,
                    const std::vector<int32_t> &g, const std::vector<uint8_t> &z) {
        Exact<uint64_t> em(m), eah(ah), eaz(az);
        Exact<int32_t> eg(g);
        Exact<uint8_t> ez(z);
        return aff_pack_pods(p, em.p, eah.p, eaz.p, eg.p, ez.p, &words, &pods);
    };
    // p outside [0, 2^30) is refused before any array is read: one-element arrays
    expect(pack(-1, {1}, {1}, {1}, {0}, {1}) != nullptr, "p -1");
    expect(pack((int64_t)1 << 30, {1}, {1}, {1}, {0}, {1}) != nullptr, "p 2^30");
    expect(pack(INT64_MAX, {1}, {1}, {1}, {0}, {1}) != nullptr, "p INT64_MAX");
    expect(pack(INT64_MIN, {1}, {1}, {1}, {0}, {1}) != nullptr, "p INT64_MIN");
    expect(pack(3, {}, {}, {}, {0, 64, 1}, {}) != nullptr, "an affinity group of 64");
    expect(pack(3, {}, {}, {}, {0, 1, -2}, {}) != nullptr, "an affinity group of -2");
    expect(pack(3, {}, {}, {}, {INT32_MAX, 1, 0}, {}) != nullptr, "an affinity group of INT32_MAX");
    expect(pack(3, {}, {}, {}, {0, 1, INT32_MIN}, {}) != nullptr, "an affinity group of INT32_MIN");
    expect(pack(0, {}, {}, {}, {}, {}) == nullptr && words.empty() && pods.empty(), "no pods");
    expect(pack(3, {}, {}, {}, {}, {}) == nullptr && words == std::vector<int32_t>(3, 0) &&
               pods == std::vector<uint64_t>(12, 0), "every array NULL: empty pods");
    expect(pack(4, {1, 0, 0, 0}, {0, 2, 0, 0}, {0, 0, 4, 0}, {-1, -1, -1, -1}, {1, 1, 1, 1}) == nullptr, "masks only");
    expect(words == std::vector<int32_t>({1, 1, 1, 0}), "masks only: the scope flag needs a term, an empty pod is 0");
    expect(pods[0] == 1 && pods[5] == 2 && pods[10] == 4 && pods[3] == 0 && pods[15] == 0, "masks only: pod-major");
    expect(pack(3, {}, {}, {}, {63, 0, -1}, {1, 0, 1}) == nullptr, "terms only");
    expect(words == std::vector<int32_t>({3, 1, 0}) && pods[3] == (uint64_t)1 << 63 && pods[7] == 1 && pods[11] == 0, "terms only: words");
    expect(pack(2, {}, {}, {}, {5, 5}, {}) == nullptr && words == std::vector<int32_t>({1, 1}), "aff_zone NULL: host scope");
    // the worked example of include/ksched.h
    expect(pack(9, {1, 1, 2, 2, 2, 1, 1, 4, 4}, {1, 1, 0, 0, 0, 1, 0, 0, 0}, {0, 0, 2, 2, 2, 0, 0, 0, 0},
                {-1, -1, 0, 0, 0, -1, -1, 2, 2}, {0, 0, 1, 1, 1, 0, 0, 0, 1}) == nullptr, "the worked example");
    expect(words == std::vector<int32_t>({1, 1, 3, 3, 3, 1, 1, 1, 3}) && pods.size() == 36 && pods[8 * 4 + 3] == 4, "... its words");
    std::printf(failures ? "%d expectation(s) failed\n" : "every expectation met\n", failures);
    return failures != 0;
}
