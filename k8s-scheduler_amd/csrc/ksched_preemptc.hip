// ksched_preemptc.hip -- ksched_preempt_constrained: ksched_preempt (ksched_preempt.hip) with the extended columns and
// the spread table in the eligibility of a node (include/ksched.h has the rules).  A dry run against the node rows, the
// bound-pod table with its two extra columns, the extended-resource table and the spread table as they stand: nothing
// is written but the workspace.
//
// ONE device function, pc_elig, says whether a pod is eligible on a node in a given state (free cpu / memory / slots,
// free extended amounts, counted pods removed).  The scan's candidate test, the scan's reprieve test and the pick
// kernel's re-walk are that function and nothing else, so they cannot disagree about a victim.
//
// The spread clause in one compare.  With C = counts[s][d] as loaded, rem = the removed pods counted in group s, mo =
// the minimum over the other domains and c = C - rem, the rule is  c + 1 - min(mo, c) <= max_skew.  max_skew >= 1
// (ksched_load_spread), so where c <= mo it holds, and where c > mo it reads c - mo <= max_skew - 1, which c <= mo
// satisfies as well: the clause is  rem >= C - mo - max_skew + 1  =: need.  pc_need gives that number per (pod, node)
// -- INT32_MIN for a pod that enforces no group, INT32_MAX on a node without the key (rem <= 1024 never reaches it) --
// and the walks keep one register of it.  C <= 2^30 and mo >= 0, so need fits 32 bits from above; it is clamped from
// below (mo is INT32_MAX where there is no other domain).
//
//   k_preemptc_min   one wave per spread group: the minimum of its D counts, the smallest count above it and the
//                    domains at the minimum, from the counts as they stand (k_dry_min's idiom; no copy to the host).
//                    mo of a node is the second where its own domain alone holds the minimum, the minimum elsewhere.
//   k_preemptc_scan  k_preempt_scan's plan: lane = node, a wave owns a 64-node block of the slot-major table, the
//                    tile's kPreemptCTile pods are wave-uniform, one upward and one downward walk over the block's slots.
//                    A slot's extended amounts and mask are loaded once and serve the whole tile, as cpu, mem and prio
//                    do.  The [S][D] counts (16 KiB at the caps) are copied to LDS once per workgroup; a lane loads
//                    its node's domain once and gathers the tile's groups' counts there.  Templated on the labels, the
//                    extended columns in use (0..4) and spread: an instantiation reads no column it does not use, and
//                    the <.., 0, false> one reads neither table.
//   k_preemptc_pick  one wave per pod: the spans' parts -> the chosen node, then that node's walk alone with readlane.
//
// The minima kernel, then two ordinary launches per chunk, in stream order.  No workgroup waits for another: no flag,
// no poll, no device-side timeout.  Integer arithmetic only (wrapping int64 sums), vector stores only.
#include <hip/hip_runtime.h>

#include "ksched_preemptc.h"

namespace ksched {

namespace {

typedef __attribute__((address_space(4))) const int64_t CI64;
typedef __attribute__((address_space(4))) const uint64_t CU64;
typedef __attribute__((address_space(4))) const int32_t CI32;

// The key's words and their reduction are ksched_preempt.hip's, restated here: that unit stays as it is, so that its
// code object does not move.
constexpr uint32_t kBias = 0x80000000u;  // prio + 2^31 as uint32: order-preserving, 0 = KSCHED_PREEMPT_NO_VICTIM_PRIO

// (mx, sc, idx) ascending: ksched_preempt's four-field order (max prio, sum, count, node), sum | count in one word
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

// What a pod asks, wave-uniform.  NX = the extended columns in use (one unused word where there is none).
template <int NX>
struct PcReq {
    int64_t rc, rm, rp;
    int64_t er[NX];
};

// A node's state for one pod: what is free with the pods taken so far gone, and how many of those the pod's group counts.
template <int NX>
struct PcFree {
    int64_t fc, fm, fp;
    int64_t fe[NX];
    int32_t rem;
};

// THE eligibility (include/ksched.h, step 2): the pod fits into what is free, every non-zero extended request is
// covered, and the spread clause holds (need: pc_need below).  The labels are no part of it: they pass with the
// candidate and no removal changes them.
template <int NE, bool SP, int NX>
__device__ __forceinline__ bool pc_elig(const PcReq<NX> &q, const PcFree<NX> &f, int32_t need) {
    bool ok = (f.fc >= q.rc) & (f.fm >= q.rm) & (f.fp >= q.rp);
#pragma unroll
    for (int r = 0; r < NE; ++r) ok &= (q.er[r] == 0) | (q.er[r] <= f.fe[r]);
    if (SP) ok &= f.rem >= need;
    return ok;
}

// A spread group's words for one pod, wave-uniform: the minimum, the second minimum, the minimum again where exactly
// one domain holds it (-1 otherwise: no count is negative) and the skew.  row < 0: the pod enforces no group.
struct PcGroup {
    int32_t row;   // the group's row of the counts, group * D
    int32_t min1, min2, uniq, skew;
    uint64_t bit;  // the group's bit of a bound pod's mask; 0: none
};

__device__ __forceinline__ PcGroup pc_group(const PreemptCArgs &A, int32_t s) {
    PcGroup g;
    g.row = -1; g.min1 = g.min2 = 0; g.uniq = -1; g.skew = 1; g.bit = 0;
    if (s >= 0) {  // s < sp_S: checked on the host
        const CI32 *w = (CI32 *)A.sp_min + s * kPreemptCMinWords;
        g.row = s * A.sp_D;
        g.min1 = w[0]; g.min2 = w[1]; g.uniq = w[2] == 1 ? w[0] : -1;
        g.skew = ((CI32 *)A.sp_skew)[s];
        g.bit = 1ull << s;
    }
    return g;
}

// need of the header comment.  dom: the node's domain (-1: no key); C: counts[group][dom] (read only where both exist).
__device__ __forceinline__ int32_t pc_need(const PcGroup &g, int32_t dom, int32_t C) {
    if (g.row < 0) return INT32_MIN;
    if (dom < 0) return INT32_MAX;
    const int32_t mo = C == g.uniq ? g.min2 : g.min1;
    const int64_t need = (int64_t)C - (int64_t)mo - (int64_t)g.skew + 1;
    return need < (int64_t)INT32_MIN ? INT32_MIN : (int32_t)need;
}

struct PcSmem {
    uint32_t mx[kPreemptWaves][kPreemptCTile];
    uint64_t sc[kPreemptWaves][kPreemptCTile];
    int32_t ix[kPreemptWaves][kPreemptCTile];
    int32_t nc[kPreemptWaves][kPreemptCTile];
};

__global__ __launch_bounds__(64) void k_preemptc_min(PreemptCArgs A) {
    const int s = blockIdx.x;
    const int32_t *row = A.sp_cnt + s * A.sp_D;
    int32_t mn = INT32_MAX;
    for (int d = threadIdx.x; d < A.sp_D; d += 64) mn = row[d] < mn ? row[d] : mn;
    mn = wave_min_i32(mn);
    int32_t m2 = INT32_MAX;  // (stays there with one domain, or all equal: mo is then never read from it, or absent)
    int64_t at = 0;
    for (int d = threadIdx.x; d < A.sp_D; d += 64) {
        const int32_t v = row[d];
        at += v == mn;
        m2 = (v != mn && v < m2) ? v : m2;
    }
    m2 = wave_min_i32(m2);
    at = wave_sum_i64(at);
    if (threadIdx.x == 0) {
        int32_t *w = A.sp_min + s * kPreemptCMinWords;
        w[0] = mn; w[1] = m2; w[2] = (int32_t)at; w[3] = 0;
    }
}

}  // namespace

// The tile's state and a slot's loads in flight stay in registers; the tile's requests are wave-uniform, and those the
// SGPRs cannot hold live in VGPR lanes, never in scratch (the resource report).
template <bool LAB, int NE, bool SP>
__global__ __launch_bounds__(kPreemptThreads, 2) void k_preemptc_scan(PreemptCArgs A) {
    constexpr int T = kPreemptCTile;
    constexpr int NX = NE > 0 ? NE : 1;
    __shared__ PcSmem sm;
    __shared__ int32_t s_cnt[SP ? KSCHED_SPREAD_MAX_CELLS : 1];
    const PreemptArgs &P = A.a;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int span = blockIdx.x;
    const int p0 = blockIdx.y * T;
    const int64_t lo = (int64_t)span * P.span_rows;  // a multiple of 256: block-aligned
    const int64_t hi = lo + P.span_rows < P.n_local ? lo + P.span_rows : P.n_local;

    if (SP) {  // sp_S * sp_D <= KSCHED_SPREAD_MAX_CELLS (ksched_load_spread)
        for (int e = threadIdx.x; e < A.sp_S * A.sp_D; e += kPreemptThreads) s_cnt[e] = A.sp_cnt[e];
        __syncthreads();
    }

    // the tile's pods, wave-uniform (pods past the chunk are never evaluated and never written)
    PcReq<NX> rq[T];
    PcGroup gr[T];
    uint64_t sel[T];
    int32_t pr[T];
    uint32_t bmx[T];
    uint64_t bsc[T];
    int32_t bix[T], nc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int p = p0 + t < P.m ? p0 + t : 0;
        rq[t].rc = ((CI64 *)P.rc)[p]; rq[t].rm = ((CI64 *)P.rm)[p]; rq[t].rp = ((CI64 *)P.rp)[p];
#pragma unroll
        for (int r = 0; r < NX; ++r) rq[t].er[r] = r < NE ? ((CI64 *)A.er)[(size_t)p * KSCHED_EXT_MAX + r] : 0;
        gr[t] = pc_group(A, SP ? ((CI32 *)A.sg)[p] : -1);
        sel[t] = LAB ? ((CU64 *)P.sel)[p] : 0;
        pr[t] = ((CI32 *)P.prio)[p];
        bmx[t] = ~0u; bsc[t] = ~0ull; bix[t] = kNoIdx; nc[t] = 0;
    }

    for (int64_t j0 = lo + wave * 64; j0 < hi; j0 += kPreemptThreads) {  // wave-uniform trip count
        const int64_t j = j0 + lane;
        const bool valid = j < hi;
        const int64_t jr = valid ? j : lo;  // lo < n_local: a row that exists
        const NodeRec &nd = P.nodes[jr];
        const int64_t a0 = nd.a[0], a1 = nd.a[1], a2 = nd.a[2];
        const uint64_t lab = LAB ? nd.labels : 0;
        int64_t ax[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) ax[r] = r < NE ? A.ext[(int64_t)r * P.n_local + jr] : 0;
        const int32_t dom = SP ? A.sp_dom[jr] : -1;  // in [-1, sp_D) (ksched_load_spread)
        const int32_t gi = (int32_t)(P.node_offset + j);
        const int64_t blk = j0 >> 6;  // j0 < n_local: a block that exists, all 64 lanes of it stored
        const int64_t e0 = ((CI64 *)P.tb.off)[blk] + lane;
        const int depth = ((CI32 *)P.tb.depth)[blk];

        // upwards: everything below the preemptor's priority gone
        PcFree<NX> fr[T];
        int32_t need[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            fr[t].fc = a0; fr[t].fm = a1; fr[t].fp = a2; fr[t].rem = 0;
#pragma unroll
            for (int r = 0; r < NX; ++r) fr[t].fe[r] = ax[r];
            need[t] = SP ? pc_need(gr[t], dom, (gr[t].row >= 0 && dom >= 0) ? s_cnt[gr[t].row + dom] : 0) : INT32_MIN;
        }
        for (int s = 0; s < depth; ++s) {
            const int64_t e = e0 + (int64_t)s * 64;
            const int64_t vc = P.tb.cpu[e], vm = P.tb.mem[e];
            const int32_t q = P.tb.prio[e];
            int64_t ve[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) ve[r] = r < NE ? A.bext[(int64_t)r * A.entries + e] : 0;
            const uint64_t mk = SP ? A.bmask[e] : 0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (p0 + t >= P.m) break;  // wave-uniform: a one-pod call pays for one pod
                const bool on = q < pr[t];
                fr[t].fc = wadd(fr[t].fc, on ? vc : 0); fr[t].fm = wadd(fr[t].fm, on ? vm : 0);
                fr[t].fp = wadd(fr[t].fp, on ? 1 : 0);
#pragma unroll
                for (int r = 0; r < NE; ++r) fr[t].fe[r] = wadd(fr[t].fe[r], on ? ve[r] : 0);
                if (SP) fr[t].rem += (on && (mk & gr[t].bit) != 0) ? 1 : 0;
            }
        }
        // the node is a candidate where the pod is eligible now; elsewhere its lane's priority bar drops below every slot
        uint32_t mx[T];
        uint64_t sc[T];
        int32_t bar[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const bool cand = valid && (!LAB || (lab & sel[t]) == sel[t]) && pc_elig<NE, SP>(rq[t], fr[t], need[t]);
            bar[t] = cand ? pr[t] : INT32_MIN;
            mx[t] = cand ? 0u : ~0u;
            sc[t] = cand ? 0ull : ~0ull;
            nc[t] += __popcll(__ballot(cand));
        }
        // downwards, most important first: reprieve what the pod can leave in place
        for (int s = depth - 1; s >= 0; --s) {
            const int64_t e = e0 + (int64_t)s * 64;
            const int64_t vc = P.tb.cpu[e], vm = P.tb.mem[e];
            const int32_t q = P.tb.prio[e];
            const uint32_t qb = (uint32_t)q ^ kBias;
            int64_t ve[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) ve[r] = r < NE ? A.bext[(int64_t)r * A.entries + e] : 0;
            const uint64_t mk = SP ? A.bmask[e] : 0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (p0 + t >= P.m) break;  // wave-uniform
                const bool on = q < bar[t];
                PcFree<NX> g;
                g.fc = wsub(fr[t].fc, vc); g.fm = wsub(fr[t].fm, vm); g.fp = wsub(fr[t].fp, 1);
#pragma unroll
                for (int r = 0; r < NX; ++r) g.fe[r] = r < NE ? wsub(fr[t].fe[r], ve[r]) : 0;
                g.rem = fr[t].rem - ((SP && (mk & gr[t].bit) != 0) ? 1 : 0);
                const bool keep = pc_elig<NE, SP>(rq[t], g, need[t]);
                const bool rep = on & keep, vic = on & !keep;
                fr[t].fc = rep ? g.fc : fr[t].fc; fr[t].fm = rep ? g.fm : fr[t].fm; fr[t].fp = rep ? g.fp : fr[t].fp;
#pragma unroll
                for (int r = 0; r < NE; ++r) fr[t].fe[r] = rep ? g.fe[r] : fr[t].fe[r];
                fr[t].rem = rep ? g.rem : fr[t].rem;
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
    if (t < T && p0 + t < P.m) {
        uint32_t m0 = sm.mx[0][t];
        uint64_t s0 = sm.sc[0][t];
        int32_t i0 = sm.ix[0][t], n = sm.nc[0][t];
        for (int w = 1; w < kPreemptWaves; ++w) {
            if (part_less(sm.mx[w][t], sm.sc[w][t], sm.ix[w][t], m0, s0, i0)) { m0 = sm.mx[w][t]; s0 = sm.sc[w][t]; i0 = sm.ix[w][t]; }
            n += sm.nc[w][t];
        }
        const size_t l = (size_t)(p0 + t) * P.spans + span;
        PreemptPart o;
        o.mx = m0; o.idx = i0; o.sc = s0;
        P.part[l] = o;
        P.part_nc[l] = n;
    }
}

// One wave per pod: the spans' parts -> the chosen node, then that node's victims in the walk's order, by pc_elig.  (No
// label check here: the chosen node passed it as a candidate.)
template <int NE, bool SP>
__global__ __launch_bounds__(64) void k_preemptc_pick(PreemptCArgs A) {
    constexpr int NX = NE > 0 ? NE : 1;
    const PreemptArgs &P = A.a;
    const int lane = threadIdx.x;
    const int p = blockIdx.x;
    uint32_t bm = ~0u;
    uint64_t bs = ~0ull;
    int32_t bi = kNoIdx;
    int64_t n = 0;
    for (int s = lane; s < P.spans; s += 64) {
        const PreemptPart e = P.part[(size_t)p * P.spans + s];
        if (part_less(e.mx, e.sc, e.idx, bm, bs, bi)) { bm = e.mx; bs = e.sc; bi = e.idx; }
        n += P.part_nc[(size_t)p * P.spans + s];
    }
    wave_part_min(bm, bs, bi);
    n = wave_sum_i64(n);
    const int32_t gi = __builtin_amdgcn_readfirstlane(bi);
    int32_t *vout = P.out_victims + (size_t)p * P.vcap;
    const bool none = gi == kNoIdx;
    if (lane == 0) {
        P.out_node[p] = none ? -1 : gi;
        P.out_nvictims[p] = none ? 0 : (int32_t)(bs & ((1u << kPreemptCntBits) - 1));
        P.out_max_prio[p] = none ? INT32_MIN : (int32_t)(bm ^ kBias);
        P.out_sum_prio[p] = none ? 0 : (int64_t)(bs >> kPreemptCntBits);
        P.out_candidates[p] = (int32_t)n;
    }
    int nv = 0;  // victims written (wave-uniform)
    if (!none) {
        const int64_t j = (int64_t)gi - P.node_offset;  // in [0, n_local): a node the scan evaluated
        const int64_t e0 = P.tb.off[j >> 6] + (j & 63);
        const int seg = P.tb.seg[j];                    // <= depth of the block: every slot below exists
        PcReq<NX> rq;
        rq.rc = P.rc[p]; rq.rm = P.rm[p]; rq.rp = P.rp[p];
#pragma unroll
        for (int r = 0; r < NX; ++r) rq.er[r] = r < NE ? A.er[(size_t)p * KSCHED_EXT_MAX + r] : 0;
        const PcGroup gr = pc_group(A, SP ? A.sg[p] : -1);
        const int32_t pr = P.prio[p];
        const NodeRec &nd = P.nodes[j];
        const int32_t dom = SP ? A.sp_dom[j] : -1;
        const int32_t need = SP ? pc_need(gr, dom, (gr.row >= 0 && dom >= 0) ? A.sp_cnt[gr.row + dom] : 0) : INT32_MIN;
        // the potential victims are the first L slots of the segment (ascending priority)
        int64_t sc_ = 0, sm_ = 0, se_[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) se_[r] = 0;
        int L = 0, rem = 0;
        for (int s0 = 0; s0 < seg; s0 += 64) {
            const int s = s0 + lane;
            const bool in = s < seg;
            const int64_t e = e0 + (int64_t)(in ? s : 0) * 64;
            const bool on = in && P.tb.prio[e] < pr;
            sc_ = wadd(sc_, on ? P.tb.cpu[e] : 0); sm_ = wadd(sm_, on ? P.tb.mem[e] : 0);
#pragma unroll
            for (int r = 0; r < NE; ++r) se_[r] = wadd(se_[r], on ? A.bext[(int64_t)r * A.entries + e] : 0);
            L += __popcll(__ballot(on));
            if (SP) rem += __popcll(__ballot(on && (A.bmask[e] & gr.bit) != 0));
        }
        PcFree<NX> fr;
        fr.fc = wadd(nd.a[0], wave_sum_i64(sc_)); fr.fm = wadd(nd.a[1], wave_sum_i64(sm_)); fr.fp = wadd(nd.a[2], (int64_t)L);
#pragma unroll
        for (int r = 0; r < NX; ++r) fr.fe[r] = r < NE ? wadd(A.ext[(int64_t)r * P.n_local + j], wave_sum_i64(se_[r])) : 0;
        fr.rem = rem;
        // the walk, from slot L - 1 down: lane k holds slot base - k, the greedy step is wave-uniform
        for (int base = L - 1; base >= 0; base -= 64) {
            const int s = base - lane;
            const int64_t e = e0 + (int64_t)(s >= 0 ? s : 0) * 64;
            const int64_t vc = P.tb.cpu[e], vm = P.tb.mem[e];
            const int32_t vt = P.tb.tidx[e];
            int64_t ve[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) ve[r] = r < NE ? A.bext[(int64_t)r * A.entries + e] : 0;
            const int32_t vb = (SP && (A.bmask[e] & gr.bit) != 0) ? 1 : 0;
            const int cnt = base + 1 < 64 ? base + 1 : 64;
            for (int k = 0; k < cnt; ++k) {
                PcFree<NX> g;
                g.fc = wsub(fr.fc, readlane_i64(vc, k)); g.fm = wsub(fr.fm, readlane_i64(vm, k)); g.fp = wsub(fr.fp, 1);
#pragma unroll
                for (int r = 0; r < NX; ++r) g.fe[r] = r < NE ? wsub(fr.fe[r], readlane_i64(ve[r], k)) : 0;
                g.rem = fr.rem - (SP ? __builtin_amdgcn_readlane(vb, k) : 0);
                const int32_t ti = __builtin_amdgcn_readlane(vt, k);
                if (pc_elig<NE, SP>(rq, g, need)) {
                    fr = g;  // reprieved
                } else {
                    if (lane == 0 && nv < P.vcap) vout[nv] = ti;
                    ++nv;
                }
            }
        }
    }
    for (int r = (nv < P.vcap ? nv : P.vcap) + lane; r < P.vcap; r += 64) vout[r] = -1;
}

namespace {

template <int NE, bool SP>
hipError_t launch_preemptc_t(bool lab, const PreemptCArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.a.spans, (unsigned)((a.a.m + kPreemptCTile - 1) / kPreemptCTile));
    if (lab) hipLaunchKernelGGL((k_preemptc_scan<true, NE, SP>), grid, dim3(kPreemptThreads), 0, s, a);
    else hipLaunchKernelGGL((k_preemptc_scan<false, NE, SP>), grid, dim3(kPreemptThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_preemptc_pick<NE, SP>), dim3((unsigned)a.a.m), dim3(64), 0, s, a);
    return hipGetLastError();
}

template <bool SP>
hipError_t launch_preemptc_ne(bool lab, const PreemptCArgs &a, hipStream_t s) {
    static_assert(KSCHED_EXT_MAX == 4, "one instantiation per column count");
    switch (a.n_ext) {
    case 0: return launch_preemptc_t<0, SP>(lab, a, s);
    case 1: return launch_preemptc_t<1, SP>(lab, a, s);
    case 2: return launch_preemptc_t<2, SP>(lab, a, s);
    case 3: return launch_preemptc_t<3, SP>(lab, a, s);
    case 4: return launch_preemptc_t<4, SP>(lab, a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_preemptc_min(const PreemptCArgs &a, hipStream_t s) {
    if (!a.sp_dom) return hipSuccess;
    hipLaunchKernelGGL(k_preemptc_min, dim3((unsigned)a.sp_S), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_preemptc(bool lab, const PreemptCArgs &a, hipStream_t s) {
    if (a.a.m <= 0 || a.a.n_local <= 0) return hipSuccess;
    return a.sp_dom ? launch_preemptc_ne<true>(lab, a, s) : launch_preemptc_ne<false>(lab, a, s);
}

}  // namespace ksched
