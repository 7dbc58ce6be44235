// ksched_rank_steps.h -- the register-only list steps of the ranked dry runs (ksched_rank.hip, ksched_dryrun.hip): a
// pod's 64-entry list is one (key code, idx) pair per lane, rank r in lane r; rank_merge_step merges two such lists,
// rank_insert_step inserts one candidate, code_key turns a key code back into the key.  Built on the wave sort of
// ksched_merge.h.
#pragma once

#include "ksched_merge.h"

namespace ksched {

// kept, cand: sorted 64-lists (rank r in lane r) over disjoint nodes.  On return kept is the sorted best 64 of
// the 128.  Lane l first keeps the better of kept[l] and cand[63 - l] (the flip of the bitonic merge: of the pairs
// (kept[l], cand[63 - l]) the winners are the best 64 of the 128), and the winners, read along the lanes, fall and
// then rise -- a bitonic sequence, which the six half-cleaners (xor 32 .. 1, the lane with the bit clear keeps
// the better) sort.  tests/test_rank_host.py runs this network, and rank_insert_step below, lane for lane over
// every zero-one input.
__device__ __forceinline__ void rank_merge_step(uint64_t &kc, int32_t &ki, uint64_t cc, int32_t ci, const int lane) {
    uint32_t lo = (uint32_t)kc, hi = (uint32_t)(kc >> 32), ix = (uint32_t)ki;
    {
        const uint32_t rlo = xpartner<63>((uint32_t)cc), rhi = xpartner<63>((uint32_t)(cc >> 32));
        const uint32_t rix = xpartner<63>((uint32_t)ci);
        const bool take = code_better(((uint64_t)rhi << 32) | rlo, (int32_t)rix, kc, ki);
        lo = take ? rlo : lo;
        hi = take ? rhi : hi;
        ix = take ? rix : ix;
    }
    sort_stage<32, 32>(lo, hi, ix, lane); sort_stage<16, 16>(lo, hi, ix, lane);
    sort_stage<8, 8>(lo, hi, ix, lane); sort_stage<4, 4>(lo, hi, ix, lane);
    sort_stage<2, 2>(lo, hi, ix, lane); sort_stage<1, 1>(lo, hi, ix, lane);
    kc = ((uint64_t)hi << 32) | lo;
    ki = (int32_t)ix;
}

// One candidate (xc, xi), wave-uniform, into the sorted list: the lanes whose entry it beats are a suffix; each of
// them takes its upper neighbour's entry (DPP wave_shr:1), the first of them the candidate; lane 63's entry falls
// off.  A candidate that beats nobody changes nothing.  Lane 0's missing neighbour reads as the unbeatable code ~0.
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v, uint32_t lane0) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)lane0, (int)v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ void rank_insert_step(uint64_t &kc, int32_t &ki, uint64_t xc, int32_t xi) {
    const uint32_t plo = wave_shr1((uint32_t)kc, 0xffffffffu), phi = wave_shr1((uint32_t)(kc >> 32), 0xffffffffu);
    const uint32_t pix = wave_shr1((uint32_t)ki, 0u);
    const uint64_t pc = ((uint64_t)phi << 32) | plo;
    const bool b = code_better(xc, xi, kc, ki);               // the candidate beats this lane's entry
    const bool pb = code_better(xc, xi, pc, (int32_t)pix);    // ... and its upper neighbour's
    kc = b ? (pb ? pc : xc) : kc;
    ki = b ? (pb ? (int32_t)pix : xi) : ki;
}

__device__ __forceinline__ double code_key(uint64_t c) {  // inverse of key_code
    const uint64_t u = (c >> 63) ? (c & 0x7fffffffffffffffull) : ~c;
    return __longlong_as_double((long long)u);
}

}  // namespace ksched
