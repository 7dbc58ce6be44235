// ksched_dryrun.hip -- ksched_rank_full / ksched_explain_full: ksched_rank and ksched_explain with
// ksched_schedule_full's eligible in the place of fits, against the node rows AND the spread, extended-resource and
// affinity tables as they stand.  Dry runs: no row and no table is written.
//
// ONE device function, dry_reason (ksched_reason.h: k_exact<kRunFullWhy> uses it too), gives the FailedScheduling code
// of a (pod, node) pair -- the first failing check in include/ksched.h's order; 0 is eligible.  The scan ranks by it, the merge labels the ranked entries with it and the
// explain kernel is nothing else, so ranking and explaining cannot disagree.
//
//   k_dry_min     one wave per spread group: the minimum of its D counts, into the call's workspace (the scan's
//                 prologue turns it into the largest count an eligible domain may hold; no copy to the host).
//   k_dry_scan    k_rank_scan's mapping (ksched_rank.hip): grid (node spans, pod tiles), lane = node, a pod's 64-entry
//                 list one (key code, idx) pair per lane, the same bar / insert / sort-and-merge steps
//                 (ksched_rank_steps.h), the waves folding through LDS.  Beside its NodeRec a lane loads its node's
//                 spread domain, extended columns, affinity domain and the two node words the predicate reads; the two
//                 tables a (pod, node) pair gathers from -- the [S][D] counts and the per-zone {member, anti} words,
//                 16 KiB each at the caps -- are copied to LDS once per workgroup.  The tile is kDryTile pods: a pod's
//                 wave-uniform state is about three times k_rank_scan's (DESIGN.md section 4.12 has the register
//                 report).  The reason histogram costs no ballot: a lane counts its own nodes in sixteen 8-bit fields
//                 of two registers per pod; every kDryFlush steps, and at the end of the span, the fields are widened
//                 to 16 bits (64 lanes x 255 < 2^16) and four wave sums reduce all sixteen.
//   k_dry_merge   one workgroup per pod: folds the span lists as k_rank_merge does, sums the spans' histograms, and
//                 recomputes each ranked node's code from its row and the tables (a few gathers per entry, from L2).
//   k_dry_explain one pod, lane = node, fourteen ballots per wave: k_explain_state's shape, the counts meeting in LDS
//                 before they go to global memory.
//
// Ordinary launches in stream order.  No workgroup waits for another: no flag, no poll, no device-side timeout.
// Scores come from pair_key_fast / price_key with the rows' hoisted reciprocals, fed the eligibility exactly as
// k_exact feeds it, so the bits agree with the scheduler by construction.
#include <hip/hip_runtime.h>

#include "ksched_dryrun.h"
#include "ksched_rank_steps.h"
#include "ksched_reason.h"  // PodU, RowX, dry_reason

namespace ksched {

namespace {

typedef __attribute__((address_space(4))) const DryPod CPod;
typedef __attribute__((address_space(4))) const int32_t CI32;

__device__ __forceinline__ PodU load_pod(const DryPod *pods, int p, const DryTables &t) {
    const CPod *q = (CPod *)pods + p;
    PodU u;
    u.rc = q->rc; u.rm = q->rm; u.rp = q->rp;
    u.sel = q->sel; u.mem = q->mem; u.anti_h = q->anti_h; u.anti_z = q->anti_z; u.abit = q->abit;
#pragma unroll
    for (int r = 0; r < KSCHED_EXT_MAX; ++r) u.er[r] = q->er[r];
    const int32_t s = t.sp_dom ? q->sgroup : -1;
    u.srow = -1; u.slim = 0;
    if (s >= 0) {
        u.srow = s * t.sp_D;
        u.slim = (int64_t)((CI32 *)t.sp_skew)[s] + (int64_t)((CI32 *)t.sp_min)[s] - 1;
    }
    u.flags = t.af_dom ? q->flags : 0;
    return u;
}

__device__ __forceinline__ RowX load_rowx(const DryTables &t, int64_t j, int64_t n) {
    RowX x;
    x.sd = t.sp_dom ? t.sp_dom[j] : -1;
#pragma unroll
    for (int r = 0; r < KSCHED_EXT_MAX; ++r) x.ext[r] = (t.ext && r < t.n_ext) ? t.ext[(int64_t)r * n + j] : 0;
    x.ad = -1; x.nm = 0; x.na = 0;
    if (t.af_dom) { x.ad = t.af_dom[j]; x.nm = t.af_mem[j]; x.na = t.af_anti_h[j]; }
    return x;
}

// The LDS of the scan and the merge: every wave's lists (scan: kDryTile pods; merge: one) and histograms.
template <int T>
struct DrySmem {
    uint64_t code[kRankWaves][T][64];
    int32_t idx[kRankWaves][T][64];
    int32_t hist[kRankWaves][T][kDryHist];
};

// A lane's sixteen 8-bit counts of one pod (code c in byte c & 7 of h[c >> 3]), summed over the wave into dst[16]
// (this wave's, in LDS) and cleared.  Even and odd bytes are widened apart into four 16-bit fields a word: no field
// can carry into its neighbour below 65536 = 64 lanes x 1024 steps, and a flush comes after at most kDryFlush.
__device__ __forceinline__ void hist_flush(uint64_t &h0, uint64_t &h1, int32_t *dst, int lane) {
    constexpr uint64_t kEven = 0x00ff00ff00ff00ffull;
    const uint64_t w[4] = {h0 & kEven, (h0 >> 8) & kEven, h1 & kEven, (h1 >> 8) & kEven};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t s = (uint64_t)wave_sum_i64((int64_t)w[i]);  // (in every lane)
        // lane q < 4 takes field q of the word: code 2 q + (i & 1), in the upper half for i >= 2
        if (lane < 4) dst[(i >> 1) * 8 + 2 * lane + (i & 1)] += (int32_t)((s >> (16 * lane)) & 0xffffu);
    }
    h0 = h1 = 0;
}

__global__ __launch_bounds__(64) void k_dry_min(DryTables t) {
    const int s = blockIdx.x;
    int32_t mn = 0x7fffffff;
    for (int d = threadIdx.x; d < t.sp_D; d += 64) {
        const int32_t v = t.sp_cnt[s * t.sp_D + d];
        mn = v < mn ? v : mn;
    }
    mn = wave_min_i32(mn);
    if (threadIdx.x == 0) t.sp_min[s] = mn;
}

}  // namespace

// 2 waves per SIMD asked for, as k_rank_scan: two workgroups per CU (2 x 45 KiB of LDS) hide one's loads behind the
// other's f64 work and leave the allocator 256 VGPRs.
template <int PRIO, int DOM, bool LAB, bool F53>
__global__ __launch_bounds__(kRankThreads, 2) void k_dry_scan(DryArgs A) {
    constexpr int T = kDryTile;
    __shared__ DrySmem<T> sm;
    __shared__ int32_t s_cnt[KSCHED_SPREAD_MAX_CELLS];
    __shared__ uint64_t s_zone[2 * KSCHED_SPREAD_MAX_DOMAINS];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int span = blockIdx.x;
    const int p0 = blockIdx.y * T;
    const int64_t lo = (int64_t)span * A.span_rows;
    const int64_t hi = lo + A.span_rows < A.n_local ? lo + A.span_rows : A.n_local;
    const double y3 = recip(3.0);

    // the two gathered tables, and this wave's histograms zeroed
    if (A.t.sp_dom)
        for (int e = threadIdx.x; e < A.t.sp_S * A.t.sp_D; e += kRankThreads) s_cnt[e] = A.t.sp_cnt[e];
    if (A.t.af_dom)
        for (int e = threadIdx.x; e < 2 * A.t.af_D; e += kRankThreads) s_zone[e] = A.t.af_zone[e];
#pragma unroll
    for (int t = 0; t < T; ++t)
        if (lane < kDryHist) sm.hist[wave][t][lane] = 0;
    __syncthreads();

    // the tile's pods, wave-uniform (pods past the chunk are pod 0 again and are never written)
    PodU pu[T];
    uint64_t kc[T], h0[T], h1[T];
    int32_t ki[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        pu[t] = load_pod(A.pods, p0 + t < A.m ? p0 + t : 0, A.t);
        kc[t] = 0ull; ki[t] = kNoIdx; h0[t] = h1[t] = 0ull;
    }

    int pending = 0;  // steps counted since the last flush
    for (int64_t j0 = lo + wave * 64; j0 < hi; j0 += kRankThreads) {  // wave-uniform trip count
        const int64_t j = j0 + lane;
        const bool valid = j < hi;
        const int64_t jr = valid ? j : lo;  // lo < n_local: a row that exists
        const NodeRec &nd = A.nodes[jr];
        const int64_t a0 = nd.a[0], a1 = nd.a[1], a2 = nd.a[2];
        const double f0 = nd.af[0], f1 = nd.af[1], f2 = nd.af[2];
        const double y0 = nd.y[0], y1 = nd.y[1], y2 = nd.y[2];
        const uint64_t lab = LAB ? nd.labels : 0;
        const float price = nd.price;
        const RowX x = load_rowx(A.t, jr, A.n_local);
        const int32_t gi = (int32_t)(A.node_offset + j);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (p0 + t >= A.m) continue;  // wave-uniform: a one-pod call pays for one pod
            const int c = dry_reason<LAB>(pu[t], a0, a1, a2, lab, x, s_cnt, s_zone);
            const bool f = valid && c == 0;
            {   // the lane's own count of code c (nothing for a lane past the span)
                const uint64_t one = valid ? 1ull << ((c & 7) * 8) : 0ull;
                h0[t] += c < 8 ? one : 0ull;
                h1[t] += c < 8 ? 0ull : one;
            }
            double key = 0.0;
            const bool el = pair_key_fast<PRIO, DOM, F53>(f, pu[t].rc, pu[t].rm, pu[t].rp, (double)pu[t].rc,
                                                          (double)pu[t].rm, (double)pu[t].rp, a0, a1, a2, f0, f1, f2, y0,
                                                          y1, y2, y3, price, &key) && valid;
            uint64_t cc = el ? key_code(key) : 0ull;
            int32_t ci = el ? gi : kNoIdx;
            // the bar: the list's last entry ((0, kNoIdx) until the list is full: every eligible pair beats it)
            const uint64_t tc = readlane_u64(kc[t], 63);
            const int32_t ti = __builtin_amdgcn_readlane(ki[t], 63);
            uint64_t q = __ballot(code_better(cc, ci, tc, ti));  // wave-uniform
            if (q != 0 && __popcll(q) <= kRankInsertMax) {
                do {  // a few rows beat the bar: one insert each
                    const int src = __ffsll((unsigned long long)q) - 1;
                    q &= q - 1;
                    rank_insert_step(kc[t], ki[t], readlane_u64(cc, src), __builtin_amdgcn_readlane(ci, src));
                } while (q != 0);
            } else if (q != 0) {
                wave_sort_desc<1>(cc, ci, lane);
                rank_merge_step(kc[t], ki[t], cc, ci, lane);
            }
        }
        if (++pending == kDryFlush) {  // before an 8-bit field can overflow
            pending = 0;
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (p0 + t < A.m) hist_flush(h0[t], h1[t], sm.hist[wave][t], lane);
        }
    }

    // fold the workgroup's waves: every wave leaves its lists and histograms in LDS, wave w merges pods w, w + 4, ...
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (p0 + t < A.m) hist_flush(h0[t], h1[t], sm.hist[wave][t], lane);
        sm.code[wave][t][lane] = kc[t];
        sm.idx[wave][t][lane] = ki[t];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < (T + kRankWaves - 1) / kRankWaves; ++u) {
        const int t = wave + u * kRankWaves;
        if (t >= T || p0 + t >= A.m) continue;  // wave-uniform
        uint64_t c = sm.code[0][t][lane];
        int32_t x = sm.idx[0][t][lane];
#pragma unroll
        for (int w = 1; w < kRankWaves; ++w) rank_merge_step(c, x, sm.code[w][t][lane], sm.idx[w][t][lane], lane);
        const size_t l = (size_t)(p0 + t) * A.spans + span;
        Cand o;
        o.key = x == kNoIdx ? -__builtin_inf() : code_key(c);
        o.idx = x;
        o.pad = 0;
        A.part[l * 64 + lane] = o;
        if (lane < kDryHist) {
            int32_t n = 0;
#pragma unroll
            for (int w = 0; w < kRankWaves; ++w) n += sm.hist[w][t][lane];
            A.part_hist[l * kDryHist + lane] = n;
        }
    }
}

// One workgroup per pod.  Wave w folds spans w, w + 4, ...; the four lists meet in LDS; wave 0 writes.  Thread x sums
// code x & 15 over the spans x >> 4, x >> 4 + 16, ...; the sixteen partial sums of a code meet in LDS too.
template <bool LAB>
__global__ __launch_bounds__(kRankThreads) void k_dry_merge(DryArgs A, int prio) {
    __shared__ DrySmem<1> sm;
    __shared__ int64_t s_hist[kRankThreads];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int p = blockIdx.x;
    const Cand *lists = A.part + (size_t)p * A.spans * 64;
    uint64_t c = 0ull;
    int32_t x = kNoIdx;
    for (int s = wave; s < A.spans; s += kRankWaves) {  // wave-uniform
        const Cand e = lists[(size_t)s * 64 + lane];
        const uint64_t ec = e.idx == kNoIdx ? 0ull : key_code(e.key);
        if (__ballot(e.idx != kNoIdx) != 0) rank_merge_step(c, x, ec, e.idx, lane);
    }
    {
        int64_t n = 0;
        const int32_t *ph = A.part_hist + (size_t)p * A.spans * kDryHist;
        for (int s = threadIdx.x >> 4; s < A.spans; s += kRankThreads / kDryHist) n += ph[(size_t)s * kDryHist + (threadIdx.x & 15)];
        s_hist[threadIdx.x] = n;
    }
    sm.code[wave][0][lane] = c;
    sm.idx[wave][0][lane] = x;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < kRankWaves; ++w) rank_merge_step(c, x, sm.code[w][0][lane], sm.idx[w][0][lane], lane);
    int64_t hn = 0;  // lane r < 16: the nodes of code r
    if (lane < kDryHist)
        for (int g = 0; g < kRankThreads / kDryHist; ++g) hn += s_hist[g * kDryHist + lane];
    if (lane < kNumReasonsFull) A.out_hist[(size_t)p * kNumReasonsFull + lane] = hn;
    const int nv = __popcll(__ballot(x != kNoIdx));  // the valid entries are a prefix
    const int cnt = nv < A.k ? nv : A.k;
    if (lane < A.k) {
        const bool ok = lane < cnt;
        int r = 0;
        double sc = 0.0;
        if (ok) {
            const int64_t j = (int64_t)x - A.node_offset;
            const NodeRec &nd = A.nodes[j];
            const PodU u = load_pod(A.pods, p, A.t);
            r = dry_reason<LAB>(u, nd.a[0], nd.a[1], nd.a[2], LAB ? nd.labels : 0, load_rowx(A.t, j, A.n_local),
                                A.t.sp_cnt, A.t.af_zone);
            const double key = code_key(c);
            sc = prio == kPrioPrice ? 0.0 - key : key;
        }
        const size_t o = (size_t)p * A.k + lane;
        A.out_idx[o] = ok ? x : -1;
        A.out_score[o] = sc;
        A.out_reason[o] = (uint8_t)r;
    }
    if (lane == 0) { A.out_count[p] = cnt; A.out_feasible[p] = (int32_t)hn; }
}

namespace {

// lane = node.  A wave's fourteen ballots meet in LDS first: with every constraint on most codes occur in most waves, and
// fourteen global atomics per wave on the same fourteen words took 108 us over c4's 100k rows; per workgroup of sixteen
// waves they are at most fourteen.
template <bool LAB>
__global__ __launch_bounds__(kDryExplainThreads) void k_dry_explain(const NodeRec *nodes, int64_t n, DryTables t, DryPod pod,
                                                                    uint8_t *reason, unsigned long long *counts) {
    __shared__ uint32_t s_cnt[kNumReasonsFull];
    if (threadIdx.x < kNumReasonsFull) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int r = -1;
    if (j < n) {
        PodU u;
        u.rc = pod.rc; u.rm = pod.rm; u.rp = pod.rp;
        u.sel = pod.sel; u.mem = pod.mem; u.anti_h = pod.anti_h; u.anti_z = pod.anti_z; u.abit = pod.abit;
#pragma unroll
        for (int e = 0; e < KSCHED_EXT_MAX; ++e) u.er[e] = pod.er[e];
        const int32_t s = t.sp_dom ? pod.sgroup : -1;
        u.srow = s >= 0 ? s * t.sp_D : -1;
        u.slim = s >= 0 ? (int64_t)t.sp_skew[s] + (int64_t)t.sp_min[s] - 1 : 0;
        u.flags = t.af_dom ? pod.flags : 0;
        const NodeRec &nd = nodes[j];
        r = dry_reason<LAB>(u, nd.a[0], nd.a[1], nd.a[2], LAB ? nd.labels : 0, load_rowx(t, j, n), t.sp_cnt, t.af_zone);
        if (reason) reason[j] = (uint8_t)r;
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kNumReasonsFull; ++k) {
        const unsigned long long m = __ballot(r == k);
        if (lane == 0 && m) atomicAdd(&s_cnt[k], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < kNumReasonsFull && s_cnt[threadIdx.x])
        atomicAdd(counts + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

template <int P_, int D_, bool L_, bool F_>
hipError_t launch_dry_rank_t(const DryArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.spans, (unsigned)((a.m + kDryTile - 1) / kDryTile));
    hipLaunchKernelGGL((k_dry_scan<P_, D_, L_, F_>), grid, dim3(kRankThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_dry_merge<L_>), dim3((unsigned)a.m), dim3(kRankThreads), 0, s, a, P_);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_dry_min(const DryTables &t, hipStream_t s) {
    if (!t.sp_dom) return hipSuccess;
    hipLaunchKernelGGL(k_dry_min, dim3((unsigned)t.sp_S), dim3(64), 0, s, t);
    return hipGetLastError();
}

hipError_t launch_dry_rank(int prio, int dom, bool lab, bool fast53, const DryArgs &a, hipStream_t s) {
    if (a.m <= 0 || a.n_local <= 0) return hipSuccess;
    KSCHED_DISPATCH(prio, dom, lab, fast53, (launch_dry_rank_t<P_, D_, L_, F_>(a, s)));
}

hipError_t launch_dry_explain(const NodeRec *nodes, int64_t n, const DryTables &t, const DryPod &pod, bool use_labels,
                              uint8_t *reason, unsigned long long *counts, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kDryExplainThreads - 1) / kDryExplainThreads)), block(kDryExplainThreads);
    if (use_labels) hipLaunchKernelGGL(k_dry_explain<true>, grid, block, 0, s, nodes, n, t, pod, reason, counts);
    else hipLaunchKernelGGL(k_dry_explain<false>, grid, block, 0, s, nodes, n, t, pod, reason, counts);
    return hipGetLastError();
}

}  // namespace ksched
