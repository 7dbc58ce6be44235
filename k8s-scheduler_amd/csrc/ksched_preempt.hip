// ksched_preempt.hip -- ksched_preempt: for each of m pods that fit nowhere, the node on which the cheapest set of
// lower-priority bound pods would have to go, and that set (include/ksched.h has the rules).  A dry run against the
// node rows and the bound-pod table (ksched_preempt.h: 64-node blocks, slot-major) as they stand: nothing is written
// but the workspace.
//
// k_rank_scan's plan: lane = node, so a wave owns one 64-node block of the table at a time and reads slot s of its 64
// segments in one coalesced access per column; the tile's kPreemptTile pods are wave-uniform and the loop over them is
// unrolled, so a slot loaded once serves every pod of the tile.
//
//   k_preempt_scan  grid (node spans, pod tiles).  Per block, two walks over its depth[b] slots.  Upwards: free[t] =
//                   alloc + every potential victim (prio_slot < prio[t]; padding carries INT32_MAX and never takes part);
//                   the node is a candidate where the pod fits into that.  Downwards, most important first: the
//                   reprieve -- the pod still fits without this slot's resources: give them back; else the slot's pod
//                   is a victim and enters the key (PreemptPart: max prio, sum | count).  Each lane keeps its best
//                   (key, node) per pod over the span's blocks; the wave's 64 are reduced by the register butterflies
//                   (wpartner), the workgroup's four through LDS: one PreemptPart and one candidate count per
//                   (pod, span).
//   k_preempt_pick  one wave per pod: reduces the spans' parts to the chosen node, then walks that node's segment alone
//                   once more -- 64 slots loaded at a time, one lane each, the greedy walk itself wave-uniform over
//                   readlane -- and writes the victims' table indices in the walk's order.  No list per (pod, node)
//                   is ever stored.
//
// Two ordinary launches in stream order.  No workgroup waits for another: no flag, no poll, no device-side timeout.
// Integer arithmetic only (wrapping int64 sums).
#include <hip/hip_runtime.h>

#include "ksched_preempt.h"

namespace ksched {

namespace {

typedef __attribute__((address_space(4))) const int64_t CI64;
typedef __attribute__((address_space(4))) const uint64_t CU64;
typedef __attribute__((address_space(4))) const int32_t CI32;

constexpr uint32_t kBias = 0x80000000u;  // prio + 2^31 as uint32: order-preserving, 0 = KSCHED_PREEMPT_NO_VICTIM_PRIO

// (mx, sc, idx) ascending: the four-field order (max prio, sum, count, node) with sum | count in one word
__device__ __forceinline__ bool part_less(uint32_t am, uint64_t as, int32_t ai, uint32_t bm, uint64_t bs, int32_t bi) {
    return am < bm || (am == bm && (as < bs || (as == bs && ai < bi)));
}

template <int S>
__device__ __forceinline__ void part_stage(uint32_t &mx, uint64_t &sc, int32_t &ix) {
    const uint32_t om = wpartner<S>(mx);
    const uint64_t os = ((uint64_t)wpartner<S>((uint32_t)(sc >> 32)) << 32) | wpartner<S>((uint32_t)sc);
    const int32_t oi = (int32_t)wpartner<S>((uint32_t)ix);
    const bool take = part_less(om, os, oi, mx, sc, ix);
    mx = take ? om : mx;
    sc = take ? os : sc;
    ix = take ? oi : ix;
}

// the wave's smallest (mx, sc, idx), in every lane
__device__ __forceinline__ void wave_part_min(uint32_t &mx, uint64_t &sc, int32_t &ix) {
    part_stage<0>(mx, sc, ix); part_stage<1>(mx, sc, ix); part_stage<2>(mx, sc, ix);
    part_stage<3>(mx, sc, ix); part_stage<4>(mx, sc, ix); part_stage<5>(mx, sc, ix);
}

__device__ __forceinline__ int64_t readlane_i64(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

struct PreemptSmem {
    uint32_t mx[kPreemptWaves][kPreemptTile];
    uint64_t sc[kPreemptWaves][kPreemptTile];
    int32_t ix[kPreemptWaves][kPreemptTile];
    int32_t nc[kPreemptWaves][kPreemptTile];
};

}  // namespace

// The tile's state (free, key, best: 13 registers a pod) and a slot's loads in flight stay in registers: 87 VGPRs at
// kPreemptTile = 4, five waves per SIMD to hide a slot's load behind the other waves' compares (the bound asks only
// for two).  The tile's requests are wave-uniform; those the 102 SGPRs cannot hold live in VGPR lanes
// (v_readlane / v_writelane), never in scratch.
template <bool LAB>
__global__ __launch_bounds__(kPreemptThreads, 2) void k_preempt_scan(PreemptArgs A) {
    constexpr int T = kPreemptTile;
    __shared__ PreemptSmem sm;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int span = blockIdx.x;
    const int p0 = blockIdx.y * T;
    const int64_t lo = (int64_t)span * A.span_rows;  // a multiple of 256: block-aligned
    const int64_t hi = lo + A.span_rows < A.n_local ? lo + A.span_rows : A.n_local;

    // the tile's pods, wave-uniform (pods past the chunk are never evaluated and never written)
    int64_t rc[T], rm[T], rp[T];
    uint64_t sel[T];
    int32_t pr[T];
    uint32_t bmx[T];
    uint64_t bsc[T];
    int32_t bix[T], nc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int p = p0 + t < A.m ? p0 + t : 0;
        rc[t] = ((CI64 *)A.rc)[p]; rm[t] = ((CI64 *)A.rm)[p]; rp[t] = ((CI64 *)A.rp)[p];
        sel[t] = LAB ? ((CU64 *)A.sel)[p] : 0;
        pr[t] = ((CI32 *)A.prio)[p];
        bmx[t] = ~0u; bsc[t] = ~0ull; bix[t] = kNoIdx; nc[t] = 0;
    }

    for (int64_t j0 = lo + wave * 64; j0 < hi; j0 += kPreemptThreads) {  // wave-uniform trip count
        const int64_t j = j0 + lane;
        const bool valid = j < hi;
        const NodeRec &nd = A.nodes[valid ? j : lo];  // lo < n_local: a row that exists
        const int64_t a0 = nd.a[0], a1 = nd.a[1], a2 = nd.a[2];
        const uint64_t lab = LAB ? nd.labels : 0;
        const int32_t gi = (int32_t)(A.node_offset + j);
        const int64_t blk = j0 >> 6;  // j0 < n_local: a block that exists, all 64 lanes of it stored
        const int64_t e0 = ((CI64 *)A.tb.off)[blk] + lane;
        const int depth = ((CI32 *)A.tb.depth)[blk];

        // upwards: everything below the preemptor's priority gone
        int64_t fc[T], fm[T], fp[T];
#pragma unroll
        for (int t = 0; t < T; ++t) { fc[t] = a0; fm[t] = a1; fp[t] = a2; }
        for (int s = 0; s < depth; ++s) {
            const int64_t e = e0 + (int64_t)s * 64;
            const int64_t vc = A.tb.cpu[e], vm = A.tb.mem[e];
            const int32_t q = A.tb.prio[e];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (p0 + t >= A.m) break;  // wave-uniform: a one-pod call pays for one pod
                const bool on = q < pr[t];
                fc[t] = wadd(fc[t], on ? vc : 0); fm[t] = wadd(fm[t], on ? vm : 0); fp[t] = wadd(fp[t], on ? 1 : 0);
            }
        }
        // the node is a candidate where the pod fits now; elsewhere its lane's priority bar drops below every slot
        uint32_t mx[T];
        uint64_t sc[T];
        int32_t bar[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const bool cand = valid && fits(rc[t], rm[t], rp[t], sel[t], fc[t], fm[t], fp[t], lab, LAB);
            bar[t] = cand ? pr[t] : INT32_MIN;
            mx[t] = cand ? 0u : ~0u;
            sc[t] = cand ? 0ull : ~0ull;
            nc[t] += __popcll(__ballot(cand));
        }
        // downwards, most important first: reprieve what the pod can leave in place
        for (int s = depth - 1; s >= 0; --s) {
            const int64_t e = e0 + (int64_t)s * 64;
            const int64_t vc = A.tb.cpu[e], vm = A.tb.mem[e];
            const int32_t q = A.tb.prio[e];
            const uint32_t qb = (uint32_t)q ^ kBias;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (p0 + t >= A.m) break;  // wave-uniform
                const bool on = q < bar[t];
                const int64_t gc = wsub(fc[t], vc), gm = wsub(fm[t], vm), gp = wsub(fp[t], 1);
                const bool keep = (gc >= rc[t]) & (gm >= rm[t]) & (gp >= rp[t]);  // (the labels passed with the candidate)
                const bool rep = on & keep, vic = on & !keep;
                fc[t] = rep ? gc : fc[t]; fm[t] = rep ? gm : fm[t]; fp[t] = rep ? gp : fp[t];
                mx[t] = (vic && qb > mx[t]) ? qb : mx[t];
                sc[t] += vic ? (((uint64_t)qb << kPreemptCntBits) + 1) : 0ull;
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int32_t ci = mx[t] == ~0u ? kNoIdx : gi;  // (a candidate's mx is a biased priority of a table pod
                                                            // below the preemptor's: never ~0)
            const bool take = part_less(mx[t], sc[t], ci, bmx[t], bsc[t], bix[t]);
            bmx[t] = take ? mx[t] : bmx[t]; bsc[t] = take ? sc[t] : bsc[t]; bix[t] = take ? ci : bix[t];
        }
    }

    // the wave's best per pod, then the workgroup's four through LDS
#pragma unroll
    for (int t = 0; t < T; ++t) {
        wave_part_min(bmx[t], bsc[t], bix[t]);
        if (lane == 0) { sm.mx[wave][t] = bmx[t]; sm.sc[wave][t] = bsc[t]; sm.ix[wave][t] = bix[t]; sm.nc[wave][t] = nc[t]; }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < T && p0 + t < A.m) {
        uint32_t m0 = sm.mx[0][t];
        uint64_t s0 = sm.sc[0][t];
        int32_t i0 = sm.ix[0][t], n = sm.nc[0][t];
        for (int w = 1; w < kPreemptWaves; ++w) {
            if (part_less(sm.mx[w][t], sm.sc[w][t], sm.ix[w][t], m0, s0, i0)) { m0 = sm.mx[w][t]; s0 = sm.sc[w][t]; i0 = sm.ix[w][t]; }
            n += sm.nc[w][t];
        }
        const size_t l = (size_t)(p0 + t) * A.spans + span;
        PreemptPart o;
        o.mx = m0; o.idx = i0; o.sc = s0;
        A.part[l] = o;
        A.part_nc[l] = n;
    }
}

// One wave per pod: the spans' parts -> the chosen node, then that node's victims in the walk's order.  (No label
// check here: the chosen node passed it as a candidate, and the reprieve never changes it.)
__global__ __launch_bounds__(64) void k_preempt_pick(PreemptArgs A) {
    const int lane = threadIdx.x;
    const int p = blockIdx.x;
    uint32_t bm = ~0u;
    uint64_t bs = ~0ull;
    int32_t bi = kNoIdx;
    int64_t n = 0;
    for (int s = lane; s < A.spans; s += 64) {
        const PreemptPart e = A.part[(size_t)p * A.spans + s];
        if (part_less(e.mx, e.sc, e.idx, bm, bs, bi)) { bm = e.mx; bs = e.sc; bi = e.idx; }
        n += A.part_nc[(size_t)p * A.spans + s];
    }
    wave_part_min(bm, bs, bi);
    n = wave_sum_i64(n);
    const int32_t gi = __builtin_amdgcn_readfirstlane(bi);
    int32_t *vout = A.out_victims + (size_t)p * A.vcap;
    const bool none = gi == kNoIdx;
    if (lane == 0) {
        A.out_node[p] = none ? -1 : gi;
        A.out_nvictims[p] = none ? 0 : (int32_t)(bs & ((1u << kPreemptCntBits) - 1));
        A.out_max_prio[p] = none ? INT32_MIN : (int32_t)(bm ^ kBias);
        A.out_sum_prio[p] = none ? 0 : (int64_t)(bs >> kPreemptCntBits);
        A.out_candidates[p] = (int32_t)n;
    }
    int nv = 0;  // victims written (wave-uniform)
    if (!none) {
        const int64_t j = (int64_t)gi - A.node_offset;  // in [0, n_local): a node the scan evaluated
        const int64_t e0 = A.tb.off[j >> 6] + (j & 63);
        const int seg = A.tb.seg[j];                    // <= depth of the block: every slot below exists
        const int64_t rc = A.rc[p], rm = A.rm[p], rp = A.rp[p];
        const int32_t pr = A.prio[p];
        const NodeRec &nd = A.nodes[j];
        // the potential victims are the first L slots of the segment (ascending priority)
        int64_t sc_ = 0, sm_ = 0;
        int L = 0;
        for (int s0 = 0; s0 < seg; s0 += 64) {
            const int s = s0 + lane;
            const bool in = s < seg;
            const int64_t e = e0 + (int64_t)(in ? s : 0) * 64;
            const bool on = in && A.tb.prio[e] < pr;
            sc_ = wadd(sc_, on ? A.tb.cpu[e] : 0); sm_ = wadd(sm_, on ? A.tb.mem[e] : 0);
            L += __popcll(__ballot(on));
        }
        int64_t fc = wadd(nd.a[0], wave_sum_i64(sc_)), fm = wadd(nd.a[1], wave_sum_i64(sm_)), fp = wadd(nd.a[2], (int64_t)L);
        // the walk, from slot L - 1 down: lane k holds slot base - k, the greedy step is wave-uniform
        for (int base = L - 1; base >= 0; base -= 64) {
            const int s = base - lane;
            const int64_t e = e0 + (int64_t)(s >= 0 ? s : 0) * 64;
            const int64_t vc = A.tb.cpu[e], vm = A.tb.mem[e];
            const int32_t vt = A.tb.tidx[e];
            const int cnt = base + 1 < 64 ? base + 1 : 64;
            for (int k = 0; k < cnt; ++k) {
                const int64_t gc = wsub(fc, readlane_i64(vc, k)), gm = wsub(fm, readlane_i64(vm, k)), gp = wsub(fp, 1);
                const int32_t ti = __builtin_amdgcn_readlane(vt, k);
                if ((gc >= rc) & (gm >= rm) & (gp >= rp)) {
                    fc = gc; fm = gm; fp = gp;  // reprieved
                } else {
                    if (lane == 0 && nv < A.vcap) vout[nv] = ti;
                    ++nv;
                }
            }
        }
    }
    for (int r = (nv < A.vcap ? nv : A.vcap) + lane; r < A.vcap; r += 64) vout[r] = -1;
}

hipError_t launch_preempt(bool lab, const PreemptArgs &a, hipStream_t s) {
    if (a.m <= 0 || a.n_local <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.spans, (unsigned)((a.m + kPreemptTile - 1) / kPreemptTile));
    if (lab) hipLaunchKernelGGL(k_preempt_scan<true>, grid, dim3(kPreemptThreads), 0, s, a);
    else hipLaunchKernelGGL(k_preempt_scan<false>, grid, dim3(kPreemptThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_preempt_pick, dim3((unsigned)a.m), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ksched
