// ksched_rank.hip -- ksched_rank: for each of m pods, the best 64 eligible nodes in the scheduler's order (key
// descending, global index ascending), against the node rows as they stand.  A dry run: no row is written.
//
// The mapping is the opposite of the stream pipeline's k_score_topk (lane = pod, rows scalar-loaded): here
// lane = node, so ONE pod already fills a wave, and a pod's list is one (key code, idx) pair per lane -- 64
// entries in 3 VGPRs, sorted and merged by the register-only wave sorts of ksched_merge.h and the list steps of
// ksched_rank_steps.h (rank_merge_step, rank_insert_step; ksched_dryrun.hip uses the same).
//
//   k_rank_scan   grid (node spans, pod tiles).  Each wave of a workgroup walks its share of the span 64 rows at
//                 a time, one NodeRec per lane, and scores the rows against the tile's kRankTile pods (wave-uniform
//                 requests, the loop fully unrolled so every list stays in registers).  Per pod it keeps the 64
//                 best pairs seen so far, rank r in lane r; lane 63 is the bar a new row must beat.  Most steps no
//                 lane beats it (one ballot); a few that do are inserted one by one (rank_insert_step); otherwise
//                 the step's 64 candidates are sorted (wave_sort_desc<1>) and merged into the list
//                 (rank_merge_step).  The workgroup's waves fold their lists through LDS and write one 64-entry
//                 Cand list and one predicate count per (pod, span).
//   k_rank_merge  one workgroup per pod: its waves fold the span lists with the same merge step, wave 0 writes the
//                 first k entries -- index, score (the key's own bits: key_code is invertible), the node's
//                 FailedScheduling reason recomputed from its row -- and the counts.
//
// Two ordinary launches in stream order.  No workgroup waits for another: no flag, no poll, no device-side
// timeout.  Scores come from fits / pair_key_fast / price_key with the rows' hoisted reciprocals, as in every
// scheduling kernel, so the bits agree with the scheduler by construction.
#include <hip/hip_runtime.h>

#include "ksched_rank.h"
#include "ksched_rank_steps.h"

namespace ksched {

namespace {

typedef __attribute__((address_space(4))) const int64_t CI64;
typedef __attribute__((address_space(4))) const uint64_t CU64;

// The LDS of both kernels: every wave's lists (scan: kRankTile pods; merge: one), and the counts.
template <int T>
struct RankSmem {
    uint64_t code[kRankWaves][T][kRankList];
    int32_t idx[kRankWaves][T][kRankList];
    int32_t fc[kRankWaves][T];
};

}  // namespace

// 2 waves per SIMD asked for: two workgroups per CU hide the row loads of one behind the other's f64 work and
// leave the allocator 256 VGPRs, so the eight lists, the row and a score's temporaries stay in registers.
template <int PRIO, int DOM, bool LAB, bool F53>
__global__ __launch_bounds__(kRankThreads, 2) void k_rank_scan(RankArgs A) {
    constexpr int T = kRankTile;
    __shared__ RankSmem<T> sm;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int span = blockIdx.x;
    const int p0 = blockIdx.y * T;
    const int64_t lo = (int64_t)span * A.span_rows;
    const int64_t hi = lo + A.span_rows < A.n_local ? lo + A.span_rows : A.n_local;
    const double y3 = recip(3.0);

    // the tile's pods, wave-uniform (pods past the chunk request nothing and are never written)
    int64_t rc[T], rm[T], rp[T];
    uint64_t sel[T];
    uint64_t kc[T];
    int32_t ki[T], fc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const bool on = p0 + t < A.m;
        const int p = on ? p0 + t : 0;
        rc[t] = ((CI64 *)A.rc)[p]; rm[t] = ((CI64 *)A.rm)[p]; rp[t] = ((CI64 *)A.rp)[p];
        sel[t] = LAB ? ((CU64 *)A.sel)[p] : 0;
        kc[t] = 0ull; ki[t] = kNoIdx; fc[t] = 0;
    }

    for (int64_t j0 = lo + wave * 64; j0 < hi; j0 += kRankThreads) {  // wave-uniform trip count
        const int64_t j = j0 + lane;
        const bool valid = j < hi;
        const NodeRec &nd = A.nodes[valid ? j : lo];  // lo < n_local: a row that exists
        const int64_t a0 = nd.a[0], a1 = nd.a[1], a2 = nd.a[2];
        const double f0 = nd.af[0], f1 = nd.af[1], f2 = nd.af[2];
        const double y0 = nd.y[0], y1 = nd.y[1], y2 = nd.y[2];
        const uint64_t lab = LAB ? nd.labels : 0;
        const float price = nd.price;
        const int32_t gi = (int32_t)(A.node_offset + j);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (p0 + t >= A.m) continue;  // wave-uniform: a one-pod call pays for one pod
            const bool f = valid && fits(rc[t], rm[t], rp[t], sel[t], a0, a1, a2, lab, LAB);
            fc[t] += __popcll(__ballot(f));
            double key = 0.0;
            const bool el = pair_key_fast<PRIO, DOM, F53>(f, rc[t], rm[t], rp[t], (double)rc[t], (double)rm[t],
                                                          (double)rp[t], a0, a1, a2, f0, f1, f2, y0, y1, y2, y3, price,
                                                          &key) && valid;
            uint64_t cc = el ? key_code(key) : 0ull;
            int32_t ci = el ? gi : kNoIdx;
            // the bar: the list's last entry ((0, kNoIdx) until the list is full: every eligible pair beats it)
            const uint64_t tc = readlane_u64(kc[t], 63);
            const int32_t ti = __builtin_amdgcn_readlane(ki[t], 63);
            uint64_t q = __ballot(code_better(cc, ci, tc, ti));  // wave-uniform
            if (q != 0 && __popcll(q) <= kRankInsertMax) {
                // a few rows beat the bar (the usual case once a list has seen some hundred rows): one insert each
                // (~20 instructions against the ~340 of a sort and a merge); a row the rising bar has overtaken
                // in the meantime beats nobody and drops out
                do {
                    const int src = __ffsll((unsigned long long)q) - 1;
                    q &= q - 1;
                    rank_insert_step(kc[t], ki[t], readlane_u64(cc, src), __builtin_amdgcn_readlane(ci, src));
                } while (q != 0);
            } else if (q != 0) {
                wave_sort_desc<1>(cc, ci, lane);
                rank_merge_step(kc[t], ki[t], cc, ci, lane);
            }
        }
    }

    // fold the workgroup's waves: every wave leaves its lists in LDS, wave w merges pods w, w + 4
#pragma unroll
    for (int t = 0; t < T; ++t) {
        sm.code[wave][t][lane] = kc[t];
        sm.idx[wave][t][lane] = ki[t];
        if (lane == 0) sm.fc[wave][t] = fc[t];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < T / kRankWaves; ++u) {
        const int t = wave + u * kRankWaves;
        if (p0 + t >= A.m) continue;  // wave-uniform
        uint64_t c = sm.code[0][t][lane];
        int32_t x = sm.idx[0][t][lane];
        int32_t n = sm.fc[0][t];
#pragma unroll
        for (int w = 1; w < kRankWaves; ++w) {
            rank_merge_step(c, x, sm.code[w][t][lane], sm.idx[w][t][lane], lane);
            n += sm.fc[w][t];
        }
        const size_t l = (size_t)(p0 + t) * A.spans + span;
        Cand o;
        o.key = x == kNoIdx ? -__builtin_inf() : code_key(c);
        o.idx = x;
        o.pad = 0;
        A.part[l * kRankList + lane] = o;
        if (lane == 0) A.part_fc[l] = n;
    }
}

// One workgroup per pod.  Wave w folds spans w, w + 4, ...; the four lists meet in LDS; wave 0 writes.
__global__ __launch_bounds__(kRankThreads) void k_rank_merge(RankArgs A, int prio, int use_labels) {
    __shared__ RankSmem<1> sm;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int p = blockIdx.x;
    const Cand *lists = A.part + (size_t)p * A.spans * kRankList;
    uint64_t c = 0ull;
    int32_t x = kNoIdx;
    for (int s = wave; s < A.spans; s += kRankWaves) {  // wave-uniform
        const Cand e = lists[(size_t)s * kRankList + lane];
        const uint64_t ec = e.idx == kNoIdx ? 0ull : key_code(e.key);
        if (__ballot(e.idx != kNoIdx) != 0) rank_merge_step(c, x, ec, e.idx, lane);
    }
    int64_t n = 0;
    for (int s = threadIdx.x; s < A.spans; s += kRankThreads) n += A.part_fc[(size_t)p * A.spans + s];
    n = wave_sum_i64(n);
    sm.code[wave][0][lane] = c;
    sm.idx[wave][0][lane] = x;
    if (lane == 0) sm.fc[wave][0] = (int32_t)n;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < kRankWaves; ++w) {
        rank_merge_step(c, x, sm.code[w][0][lane], sm.idx[w][0][lane], lane);
        n += sm.fc[w][0];
    }
    const int nv = __popcll(__ballot(x != kNoIdx));  // the valid entries are a prefix
    const int cnt = nv < A.k ? nv : A.k;
    if (lane < A.k) {
        const bool ok = lane < cnt;
        int r = 0;
        double sc = 0.0;
        if (ok) {
            const NodeRec &nd = A.nodes[(int64_t)x - A.node_offset];
            // first failing check in k_explain's order
            r = nd.a[0] < A.rc[p] ? 1 : nd.a[1] < A.rm[p] ? 2 : nd.a[2] < A.rp[p] ? 3
                : (use_labels && (nd.labels & A.sel[p]) != A.sel[p]) ? 4 : 0;
            const double key = code_key(c);
            sc = prio == kPrioPrice ? 0.0 - key : key;
        }
        const size_t o = (size_t)p * A.k + lane;
        A.out_idx[o] = ok ? x : -1;
        A.out_score[o] = sc;
        A.out_reason[o] = (uint8_t)r;
    }
    if (lane == 0) { A.out_count[p] = cnt; A.out_feasible[p] = (int32_t)n; }
}

namespace {

template <int P_, int D_, bool L_, bool F_>
hipError_t launch_rank_t(const RankArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.spans, (unsigned)((a.m + kRankTile - 1) / kRankTile));
    hipLaunchKernelGGL((k_rank_scan<P_, D_, L_, F_>), grid, dim3(kRankThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rank_merge, dim3((unsigned)a.m), dim3(kRankThreads), 0, s, a, P_, (int)L_);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rank(int prio, int dom, bool lab, bool fast53, const RankArgs &a, hipStream_t s) {
    if (a.m <= 0 || a.n_local <= 0) return hipSuccess;
    KSCHED_DISPATCH(prio, dom, lab, fast53, (launch_rank_t<P_, D_, L_, F_>(a, s)));
}

}  // namespace ksched
