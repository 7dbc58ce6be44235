// gang_check_main.cpp -- csrc/ksched_gang.h on its own, for a CPU sanitizer run of the gang checks and packing that
// ksched_schedule_gangs and ksched_schedule_constrained share (no device call, no library):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ik8s-scheduler_amd/csrc
//       tests/diag/gang_check_main.cpp -o gang_check; ./gang_check
// Every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a report.
// The last group restates ksched_schedule_constrained's order (p in [0, 2^30) before the gangs), under which p and
// n_gangs of INT64_MAX never reach an array.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ksched_gang.h"

using namespace ksched;

static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

// heap copies of exactly the given length (ASan's redzones sit right behind them); an empty list is a null pointer
static const char *check(int64_t p, int64_t n_gangs, const std::vector<int64_t> &off, const std::vector<int32_t> &mins,
                         bool with_min = true) {
    int64_t *o = off.empty() ? nullptr : (int64_t *)std::malloc(off.size() * 8);
    int32_t *m = (!with_min || mins.empty()) ? nullptr : (int32_t *)std::malloc(mins.size() * 4);
    for (size_t i = 0; i < off.size(); ++i) o[i] = off[i];
    if (m) for (size_t i = 0; i < mins.size(); ++i) m[i] = mins[i];
    const char *why = gang_check(p, n_gangs, o, m);
    std::free(o);
    std::free(m);
    return why;
}

// ksched_schedule_constrained's order
static const char *constrained(int64_t p, int64_t n_gangs, const std::vector<int64_t> &off) {
    if (p < 0 || p >= ((int64_t)1 << 30)) return "p must be in [0, 2^30)";
    if (off.empty()) return n_gangs != 0 ? "n_gangs must be 0 without gang_off" : nullptr;
    return check(p, n_gangs, off, {}, false);
}

int main() {
    const int64_t kMax = INT64_MAX;
    // p and n_gangs of 0, -1 and INT64_MAX with one-element arrays
    expect(check(0, 0, {0}, {1}) == nullptr, "p 0, no gangs");
    expect(check(0, 0, {1}, {1}) != nullptr, "p 0, gang_off[0] != 0");
    expect(check(-1, 0, {0}, {1}) != nullptr, "p -1");
    expect(check(0, -1, {0}, {1}) != nullptr, "n_gangs -1");
    expect(check(-1, -1, {0}, {1}) != nullptr, "p -1, n_gangs -1");
    expect(check(0, kMax, {0}, {1}) != nullptr, "n_gangs INT64_MAX above p 0");
    expect(check(5, kMax, {0}, {1}) != nullptr, "n_gangs INT64_MAX above p 5");
    expect(check(kMax, 0, {0}, {1}) != nullptr, "p INT64_MAX, no gangs: gang_off[0] != p");
    expect(check(kMax, 0, {kMax}, {1}) != nullptr, "p INT64_MAX, gang_off[0] == p != 0");
    expect(check(5, 0, {}, {}) != nullptr, "a null gang_off");
    // offsets that decrease, repeat or overrun
    expect(check(5, 3, {0, 2, 4, 5}, {}) == nullptr, "the worked example's gangs");
    expect(check(5, 3, {0, 2, 4, 5}, {2, 1, 1}) == nullptr, "... with minima");
    expect(check(5, 3, {0, 3, 2, 5}, {}) != nullptr, "an offset that decreases");
    expect(check(5, 3, {0, 2, 2, 5}, {}) != nullptr, "an offset that repeats");
    expect(check(5, 2, {0, 800, 5}, {}) != nullptr, "an offset beyond p, then back");
    expect(check(5, 3, {0, 3, 900, 5}, {}) != nullptr, "a later offset beyond p");
    expect(check(5, 2, {0, -5, 5}, {}) != nullptr, "a negative offset");
    expect(check(5, 2, {0, (int64_t)1 << 62, 5}, {}) != nullptr, "an offset of 2^62");
    expect(check(5, 2, {0, 2, 4}, {}) != nullptr, "the last offset short of p");
    expect(check(5, 2, {0, 2, 6}, {}) != nullptr, "the last offset beyond p");
    expect(check(5, 2, {1, 2, 5}, {}) != nullptr, "a first offset of 1");
    // the cap
    expect(check(1100, 2, {0, 1024, 1100}, {}) == nullptr, "a gang of KSCHED_GANG_MAX");
    expect(check(1100, 2, {0, 1025, 1100}, {}) != nullptr, "a gang of 1025");
    // minima of 0 and size + 1
    expect(check(1100, 2, {0, 1024, 1100}, {1024, 76}) == nullptr, "minima equal to the sizes");
    expect(check(1100, 2, {0, 1024, 1100}, {1, 1}) == nullptr, "minima of 1");
    expect(check(1100, 2, {0, 1024, 1100}, {0, 76}) != nullptr, "a minimum of 0");
    expect(check(1100, 2, {0, 1024, 1100}, {1024, 77}) != nullptr, "a minimum of size + 1");
    expect(check(1100, 2, {0, 1024, 1100}, {-1, 76}) != nullptr, "a minimum of -1");
    expect(check(1100, 2, {0, 1024, 1100}, {INT32_MIN, 76}) != nullptr, "a minimum of INT32_MIN");
    expect(check(1100, 2, {0, 1024, 1100}, {1024, INT32_MAX}) != nullptr, "a minimum of INT32_MAX");
    // the packing: 0, or size | minimum << 16 at each gang's last member, into exactly p words
    std::vector<int32_t> gend;
    const int64_t off[] = {0, 1024, 1100};
    const int32_t mins[] = {512, 76};
    gang_pack_ends(1100, 2, off, mins, &gend);
    expect(gend.size() == 1100 && gend[1023] == (1024 | 512 << 16) && gend[1099] == (76 | 76 << 16), "pack with minima");
    int64_t nz = 0;
    for (int32_t v : gend) nz += v != 0;
    expect(nz == 2, "pack: every other word is 0");
    gang_pack_ends(1100, 2, off, nullptr, &gend);
    expect(gend[1023] == (1024 | 1024 << 16) && (gend[1023] >> 16) == 1024 && (gend[1023] & 0xffff) == 1024, "pack, all required");
    gang_pack_ends(0, 0, off, nullptr, &gend);
    expect(gend.empty(), "pack of no pods");
    gang_pack_singles(3, &gend);
    expect(gend.size() == 3 && gend[0] == (1 | 1 << 16) && gend[2] == (1 | 1 << 16), "gangs of one");
    gang_pack_singles(0, &gend);
    expect(gend.empty(), "gangs of one, no pods");
    // ksched_schedule_constrained's order: p's range first
    expect(constrained(kMax, kMax, {0}) != nullptr, "constrained: p and n_gangs INT64_MAX");
    expect(constrained((int64_t)1 << 30, 1, {0}) != nullptr, "constrained: p 2^30");
    expect(constrained(-1, -1, {0}) != nullptr, "constrained: p -1");
    expect(constrained(5, 1, {}) != nullptr, "constrained: gang_off NULL with n_gangs 1");
    expect(constrained(5, -1, {}) != nullptr, "constrained: gang_off NULL with n_gangs -1");
    expect(constrained(5, 0, {}) == nullptr, "constrained: gangs off");
    expect(constrained(0, 0, {0}) == nullptr, "constrained: no pods");
    expect(constrained(5, 3, {0, 2, 4, 5}) == nullptr, "constrained: the worked example's gangs");
    std::printf(failures ? "%d expectation(s) failed\n" : "every expectation met\n", failures);
    return failures != 0;
}
