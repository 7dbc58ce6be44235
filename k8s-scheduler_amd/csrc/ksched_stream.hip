// ksched_stream.hip -- the stream pipeline's kernels (ksched_stream.h lists them; k_commit_spc: ksched_commit_spc.hip)
// and, below them, one variant lookup per dispatched kernel, which its launcher and its attribute query both go
// through.  Compiled with -ffp-contract=off: every double op rounds individually, exactly like the Go reference.
#include <hip/hip_runtime.h>

#include <mutex>
#include <set>
#include <utility>

#include "ksched_merge.h"
#include "ksched_stream.h"

namespace ksched {

// ------------------------------------------------------------------------------------------------
// Batched mode, stage 1: fused predicate + score + top-KC per (pod, workgroup).  Lane = pod of the
// batch.  A workgroup is kScoreWaves waves; wave w of workgroup g scans sub-chunk s = g + G*w of the
// NSC = G*kScoreWaves sub-chunks, i.e. the nodes j with j mod NSC == s: workgroup g holds the nodes
// j = g (mod G), so the lowest-index members of a tie class land in different workgroups and short
// lists still merge into a long exact prefix.  Node rows are wave-uniform (scalar loads of the 96-B
// NodeRec, reciprocals included).
//   Each wave keeps a sorted top-KC per lane (branch-free register insert; nodes arrive in ascending
//   index, so a strict key compare keeps ties in index order).  The wave lists fold pairwise through
//   LDS into one list per (pod, workgroup): two lists that are each cut when full fold into the top-KC
//   of their union, again cut when full.
// ------------------------------------------------------------------------------------------------
template <int KC, int PRIO, int DOM, bool LAB, bool F53>
__device__ __forceinline__ void score_topk_body(const ScoreArgs &A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *s_key = reinterpret_cast<double *>(smem);                                   // [W/2][KC][64]
    int32_t *s_idx = reinterpret_cast<int32_t *>(smem + (size_t)(kScoreWaves / 2) * KC * 64 * 8);
    int32_t *s_cnt = s_idx + (size_t)(kScoreWaves / 2) * KC * 64;                        // [64]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t G = gridDim.x;
    const int64_t NSC = G * kScoreWaves;
    const int64_t sub = (int64_t)blockIdx.x + G * wave;
    if (A.wait_committed) {
        // commit(b-2) published its plan for this batch, its commits (XBuf) and Ctl::committed with an
        // agent release: one lane polls (relaxed, s_sleep), one agent acquire, then plain loads
        __shared__ int s_late;
        if (threadIdx.x == 0) {
            const uint64_t t0 = wall_clock64();
            s_late = 0;
            while (__hip_atomic_load(A.wait_committed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < A.wait_target) {
                __builtin_amdgcn_s_sleep(1);
                if (wall_clock64() - t0 > 200000000ull) {  // 2 s: report instead of spinning forever
                    __hip_atomic_store(A.err, kErrStreamScoreWait, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    s_late = 1;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if (s_late) return;
    }
    // Batch b-2's commits (<= 128 nodes, two per lane): the wave whose sub-chunk holds a node writes it
    // back to the row (for the next launches) and overlays it on what it reads in this launch, so no
    // separate apply kernel has to run between commit(b-2) and score(b).
    int64_t pj0 = -1, pj1 = -1;  // local node index of entries lane and lane + 64, if in this sub-chunk
    {
        const int np = A.patch->count;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = h * 64 + lane;
            const int64_t j = e < np ? (int64_t)A.patch->e[e].idx - A.node_offset : -1;
            const bool mine = j >= 0 && j < A.n_local && (j % NSC) == sub;
            if (mine && blockIdx.y == 0) {
                const XRec &x = A.patch->e[e];
                set_node(A.nodes + j, x.cur[0], x.cur[1], x.cur[2]);
            }
            if (h == 0) pj0 = mine ? j : -1;
            else pj1 = mine ? j : -1;
        }
    }
    const bool anyp = __ballot(pj0 >= 0 || pj1 >= 0) != 0;
    if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
    const int64_t p0 = *A.cursor;
    if (p0 < 0 || p0 >= A.pods.p) return;  // workgroup-uniform
    __syncthreads();
    const int b = blockIdx.y * 64 + lane;
    const int64_t pod = p0 + b;
    const bool active = (b < A.B) && (pod < A.pods.p);
    const int64_t rc = active ? A.pods.rc[pod] : 0;
    const int64_t rm = active ? A.pods.rm[pod] : 0;
    const int64_t rp = active ? A.pods.rp[pod] : 0;
    const uint64_t sel = (LAB && active) ? A.pods.sel[pod] : 0;
    const double rcf = (double)rc, rmf = (double)rm, rpf = (double)rp;
    const double y3 = recip(3.0);

    double key[KC];
    int32_t idx[KC];
#pragma unroll
    for (int q = 0; q < KC; ++q) { key[q] = -__builtin_inf(); idx[q] = kNoIdx; }
    int32_t cnt = 0;
    // one node against this lane's pod: predicate, key, sorted insert (strict '>': nodes arrive in
    // ascending index, so equal keys keep index order)
    auto visit = [&](int64_t j, int64_t ac, int64_t am, int64_t ap, double af0, double af1, double af2, double y0,
                     double y1, double y2, uint64_t lab, float price) {
        const bool f = fits(rc, rm, rp, sel, ac, am, ap, lab, LAB);
        cnt += f;
        double k;
        const bool el = pair_key_fast<PRIO, DOM, F53>(f, rc, rm, rp, rcf, rmf, rpf, ac, am, ap, af0, af1, af2, y0, y1,
                                                      y2, y3, price, &k);
        double ck = el ? k : -__builtin_inf();
        int32_t ci = (int32_t)(A.node_offset + j);
        bool moved = false;  // once placed, every later entry shifts down one slot
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            const bool sw = moved || ck > key[q];
            moved = sw;
            const double tk = key[q];
            const int32_t ti = idx[q];
            key[q] = sw ? ck : tk; idx[q] = sw ? ci : ti;
            ck = sw ? tk : ck; ci = sw ? ti : ci;
        }
    };
    if (!anyp) {
        // Node rows are wave-uniform: read through the constant address space they arrive as scalar
        // loads (s_load_dwordx16 + x8) into SGPRs, one row ahead of its use -- row j + NSC is in flight
        // while row j is scored -- and feed the VALU as scalar operands (no row VGPRs).
        const NodeRecC *rows = (const NodeRecC *)(A.nodes);
        NodeRec nxt;
        if (sub < A.n_local) nxt = load_row(rows + sub);
        for (int64_t j = sub; j < A.n_local; j += NSC) {
            const NodeRec nd = nxt;
            const int64_t jn = j + NSC;
            if (jn < A.n_local) nxt = load_row(rows + jn);
            visit(j, nd.a[0], nd.a[1], nd.a[2], nd.af[0], nd.af[1], nd.af[2], nd.y[0], nd.y[1], nd.y[2], nd.labels,
                  nd.price);
        }
    } else {
        // this sub-chunk holds nodes committed by batch b-2 (~6 % of the waves at B = 64): their rows
        // are overlaid from the XBuf as they are reached (the write-back above may not be visible yet
        // to this launch's reads, and is not done at all by pod groups y > 0)
        for (int64_t j = sub; j < A.n_local; j += NSC) {
            const NodeRec &nd = A.nodes[j];
            int64_t ac = nd.a[0], am = nd.a[1], ap = nd.a[2];
            double af0 = nd.af[0], af1 = nd.af[1], af2 = nd.af[2], y0 = nd.y[0], y1 = nd.y[1], y2 = nd.y[2];
            const uint64_t hit = __ballot(pj0 == j || pj1 == j);
            if (hit) {
                const int src = __ffsll((unsigned long long)hit) - 1;
                const int e = __builtin_amdgcn_readlane(pj0 == j ? lane : lane + 64, src);
                const XRec &xr = A.patch->e[e];
                ac = xr.cur[0]; am = xr.cur[1]; ap = xr.cur[2];
                af0 = (double)ac; af1 = (double)am; af2 = (double)ap;
                y0 = recip_or_zero(ac, af0); y1 = recip_or_zero(am, af1); y2 = recip_or_zero(ap, af2);
            }
            visit(j, ac, am, ap, af0, af1, af2, y0, y1, y2, nd.labels, nd.price);
        }
    }
    if (cnt) atomicAdd(&s_cnt[lane], cnt);
    // fold the wave lists pairwise: W -> W/2 -> ... -> 1
#pragma unroll
    for (int half = kScoreWaves / 2; half >= 1; half >>= 1) {
        if (wave >= half && wave < 2 * half) {
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                s_key[((wave - half) * KC + q) * 64 + lane] = key[q];
                s_idx[((wave - half) * KC + q) * 64 + lane] = idx[q];
            }
        }
        __syncthreads();
        if (wave < half) {
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                const int32_t oi = s_idx[(wave * KC + q) * 64 + lane];
                if (oi == kNoIdx) break;
                list_insert_ordered<KC>(key, idx, s_key[(wave * KC + q) * 64 + lane], oi);
            }
        }
        __syncthreads();
    }
    if (wave == 0 && active) {
        Cand *dst = A.part + ((size_t)b * G + blockIdx.x) * KC;
#pragma unroll
        for (int q = 0; q < KC; ++q) { dst[q].key = key[q]; dst[q].idx = idx[q]; dst[q].pad = 0; }
        A.part_cnt[(size_t)b * G + blockIdx.x] = s_cnt[lane];
    }
}

template <int KC, int K>
__global__ __launch_bounds__(kMergeThreads) void k_merge_pod(MergeArgs A) {
    __shared__ MergeSmem<KC, K, kMergeThreads> sm;
    merge_pod_body<KC, K, false, kMergeThreads>(A, blockIdx.x, threadIdx.x, sm, BlockSync{});
}

// Score kernel (the merge waits on a stream event).
// <= 64 VGPRs (launch bound: 8 waves per SIMD): two score waves + two commit waves (190 VGPRs) must
// fit one SIMD, or the single-workgroup commit cannot dispatch beside the score grid.
template <int KC, int PRIO, int DOM, bool LAB, bool F53>
__global__ __launch_bounds__(kScoreThreads, 8) void k_score_topk(ScoreArgs A) {
    score_topk_body<KC, PRIO, DOM, LAB, F53>(A);
}

// ------------------------------------------------------------------------------------------------
// Rank merge: one wave per pod over the ranks' sorted Rec lists of K entries.  Each lane stages one rank's list in
// LDS; K rounds of wave arg-best over the lanes' heads (the winning lane advances); the winners' Rec rows are copied.
// Exact prefix ("cut") rule: a cut input list has unlisted candidates, all ranking below its last
// entry.  The output keeps only entries ranking at or above the best such cutoff (anything below it
// could be preceded by an unlisted candidate) and is itself cut when any input was, or when entries
// were left over after K rounds.  The flag travels in entry 0's pad.
// ------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(64) void k_merge(MergeArgs A) {
    __builtin_amdgcn_s_setprio(3);  // latency-critical: win issue arbitration over co-resident score waves
    __shared__ double s_key[64 * K];
    __shared__ int32_t s_idx[64 * K];
    const int lane = threadIdx.x;
    const int grp = blockIdx.x;
    const int b = blockIdx.y;
    const int64_t p0 = *A.cursor;
    if (p0 < 0 || p0 >= A.P || b >= A.B || p0 + b >= A.P) return;
    const int list = grp * 64 + lane;
    const bool has = list < A.C_in;
    int64_t cnt = 0;
    int n = 0;          // valid entries of this lane's list
    bool cut = false;   // this lane's list is cut
    if (has) {
        const char *blk = static_cast<const char *>(A.in) + (size_t)list * A.rank_stride;
        const Rec *src = reinterpret_cast<const Rec *>(blk) + (size_t)b * K;
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const bool v = src[q].valid != 0;
            s_key[lane * K + q] = v ? src[q].key : -__builtin_inf();
            s_idx[lane * K + q] = v ? src[q].idx : kNoIdx;
            n += v;
        }
        cut = src[0].pad != 0;
        cnt = reinterpret_cast<const int64_t *>(blk + (size_t)A.B * K * sizeof(Rec))[b];
    }
    cnt = wave_sum_i64(cnt);
    // best cutoff over the cut lists (their last valid entry)
    double ck = (cut && n > 0) ? s_key[lane * K + n - 1] : -__builtin_inf();
    int32_t ci = (cut && n > 0) ? s_idx[lane * K + n - 1] : kNoIdx;
    const bool anycut = __ballot(cut) != 0;
    {
        int32_t aux = 0;
        wave_argbest(ck, ci, aux);
    }
    __syncthreads();
    int h = 0;
    double mk = -__builtin_inf();
    int32_t mi = kNoIdx, msrc = -1;
    for (int r = 0; r < K; ++r) {
        double k = (h < n) ? s_key[lane * K + h] : -__builtin_inf();
        int32_t ix = (h < n) ? s_idx[lane * K + h] : kNoIdx;
        int32_t src = lane * K + h;
        wave_argbest(k, ix, src);
        if (ix == kNoIdx) break;  // wave-uniform
        if (src == lane * K + h) ++h;
        if (lane == r) { mk = k; mi = ix; msrc = src; }
    }
    const bool left = __ballot(h < n) != 0;  // candidates beyond the K output entries
    // entries ranking below the best cutoff are not exact
    if (anycut && mi != kNoIdx && better(ck, ci, mk, mi)) { mk = -__builtin_inf(); mi = kNoIdx; }
    const int32_t cut_out = (anycut || left) ? 1 : 0;
    if (lane < K) {
        Rec r{};
        if (mi != kNoIdx) {
            const int srcl = msrc / K, srcq = msrc % K;
            const char *blk = static_cast<const char *>(A.in) + (size_t)(grp * 64 + srcl) * A.rank_stride;
            r = reinterpret_cast<const Rec *>(blk)[(size_t)b * K + srcq];
        } else {
            r.key = -__builtin_inf(); r.idx = kNoIdx; r.valid = 0;
        }
        r.pad = lane == 0 ? cut_out : 0;
        A.out_rec[(size_t)b * K + lane] = r;
    }
    if (lane == 0) A.out_fc[b] = cnt;
}

// ------------------------------------------------------------------------------------------------
// Ordered commit of one batch: a single-wave sequencer.  For pod i of the batch, with T = nodes
// committed by pods < i of this batch (LDS table; s0 = snapshot state, cur = current state):
//   fc   = fc0[i] - sum_T fits(s0) + sum_T fits(cur)                          (predicate count)
//   t*   = best of T re-scored at cur;  u* = first list entry not in T (exact: untouched)
//   list full and all touched: t* must beat list[K-1] (every unlisted untouched node ranks below
//   it), otherwise the batch stops before pod i (overflow) and the next batch restarts there.
// One wave, no barriers: reductions are register butterflies (DPP + permlane swaps) and ballots;
// every lane evaluates the (wave-uniform) decision; requests and feasible counts are staged into LDS
// once; lane q < K holds candidate q of the current pod while the next pod's candidates load into
// the other register buffer (the loop is unrolled by two so the wait lands one pod later).
// ------------------------------------------------------------------------------------------------
constexpr int kMaxTouchedSlots = 4;  // touched nodes per lane -> 256 (previous batch's + this batch's, B <= 128)

struct CommitCtx {
    int32_t *hkey;       // open-addressing set of touched node indices (kTouchHash slots, -1 = empty)
    uint32_t *filt;      // 64K-bit filter: bit (idx & 0xffff) set once idx is touched
    Touched *T;
    const PodStage *PS;
    const CandStage *CS; // [B][K] staged candidate lists
    int nT;
    int64_t placed;
    double y3;
    int lane;
    int64_t p0;
};

__device__ __forceinline__ uint64_t stamp() {
    uint64_t t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

__device__ __forceinline__ uint32_t thash(int32_t idx) { return ((uint32_t)idx * 2654435761u) >> (32 - kTouchHashBits); }

__device__ __forceinline__ bool touched_has(const CommitCtx &cx, int32_t idx) {
    if (!(cx.filt[((uint32_t)idx & 0xffffu) >> 5] & (1u << ((uint32_t)idx & 31)))) return false;
    for (uint32_t h = thash(idx);; h = (h + 1) & (kTouchHash - 1)) {
        const int32_t k = cx.hkey[h];
        if (k == idx) return true;
        if (k < 0) return false;
    }
}

__device__ __forceinline__ void touched_insert(CommitCtx &cx, int32_t idx) {
    uint32_t h = thash(idx);
    while (cx.hkey[h] >= 0) h = (h + 1) & (kTouchHash - 1);
    cx.hkey[h] = idx;
    cx.filt[((uint32_t)idx & 0xffffu) >> 5] |= 1u << ((uint32_t)idx & 31);
}

// Touched-node re-scoring, filtered: an upper bound (reciprocal multiplies, no corrections) per slot
// decides which touched nodes could beat the threshold (thk, thi); only those are scored exactly.
// Non-candidates provably rank below the threshold, so the decision is unchanged.
// Feasibility deltas (exact integer compares) come through ballots.
template <int NS, int PRIO, int DOM, bool LAB, bool F53>
__device__ __forceinline__ void rescore_touched(const CommitCtx &cx, int64_t rc, int64_t rm, int64_t rp, uint64_t sel,
                                                double rcf, double rmf, double rpf, double thk, int32_t thi,
                                                int64_t &df, double &tk, int32_t &ti, int32_t &ts, bool &any) {
    bool cand[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int t = cx.lane + 64 * s;
        const bool in = t < cx.nT;
        const Touched &x = cx.T[in ? t : 0];
        const bool f0 = in && fits(rc, rm, rp, sel, x.s0[0], x.s0[1], x.s0[2], x.labels, LAB);
        const bool f1 = in && fits(rc, rm, rp, sel, x.cur[0], x.cur[1], x.cur[2], x.labels, LAB);
        df += (int64_t)__popcll(__ballot(f1)) - (int64_t)__popcll(__ballot(f0));
        bool c;
        if (PRIO == kPrioPrice) {
            c = f1 && better(price_key(x.price), x.idx, thk, thi);
        } else {
            bool near1;
            const double hi = resource_score_upper<F53>(rc, rm, rp, rcf, rmf, rpf, x.cur[0], x.cur[1], x.cur[2],
                                                        x.curf[0], x.curf[1], x.curf[2], x.cury[0], x.cury[1],
                                                        x.cury[2], cx.y3, &near1);
            c = in && (DOM == kDomAll || f1) && (near1 || (hi > 0.0 && hi >= thk));
        }
        cand[s] = c;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (__ballot(cand[s]) == 0) continue;  // wave-uniform: nothing to score exactly in this slot
        any = true;
        if (cand[s]) {
            const int t = cx.lane + 64 * s;
            const Touched &x = cx.T[t];
            const bool f1 = fits(rc, rm, rp, sel, x.cur[0], x.cur[1], x.cur[2], x.labels, LAB);
            double k;
            if (pair_key_fast<PRIO, DOM, F53>(f1, rc, rm, rp, rcf, rmf, rpf, x.cur[0], x.cur[1], x.cur[2], x.curf[0],
                                              x.curf[1], x.curf[2], x.cury[0], x.cury[1], x.cury[2], cx.y3, x.price,
                                              &k) &&
                better(k, x.idx, tk, ti)) {
                tk = k; ti = x.idx; ts = t;
            }
        }
    }
}

template <int K, int PRIO, int DOM, bool LAB, bool F53, bool ST>
__device__ __forceinline__ bool commit_step(const CommitArgs &A, CommitCtx &cx, int i, const PodStage &ps,
                                            const CandStage &my, uint64_t *ph) {
    const int lane = cx.lane;
    uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    if (ST) t0 = stamp();
    const int64_t rc = ps.rc, rm = ps.rm, rp = ps.rp;
    const uint64_t sel = ps.sel;
    const double rcf = (double)rc, rmf = (double)rm, rpf = (double)rp;
    // candidate list: valid prefix, first entry not committed in this batch
    const bool valid = lane < K && my.idx != kNoIdx;
    const bool untouched = valid && (cx.nT == 0 || !touched_has(cx, my.idx));
    const uint64_t vmask = __ballot(valid);
    const uint64_t umask = __ballot(untouched);
    const int cv = __popcll(vmask);
    const int uq = umask ? __ffsll((unsigned long long)umask) - 1 : K;
    const bool cut = ps.cut != 0;  // unlisted candidates exist, all ranking below the last valid entry
    // threshold a touched node must beat to matter: u*, else the last valid entry (cut list), else anything
    double thk = -__builtin_inf();
    int32_t thi = kNoIdx;
    if (uq < cv) { thk = readlane_f64(my.key, uq); thi = __builtin_amdgcn_readlane(my.idx, uq); }
    else if (cut && cv > 0) { thk = readlane_f64(my.key, cv - 1); thi = __builtin_amdgcn_readlane(my.idx, cv - 1); }
    // re-score the nodes already committed (this batch's and the previous batch's)
    int64_t df = 0;
    double tk = -__builtin_inf();
    int32_t ti = kNoIdx, ts = -1;
    bool any = false;
    if (cx.nT > 0) {
        if (cx.nT <= 64)
            rescore_touched<1, PRIO, DOM, LAB, F53>(cx, rc, rm, rp, sel, rcf, rmf, rpf, thk, thi, df, tk, ti, ts, any);
        else if (cx.nT <= 128)
            rescore_touched<2, PRIO, DOM, LAB, F53>(cx, rc, rm, rp, sel, rcf, rmf, rpf, thk, thi, df, tk, ti, ts, any);
        else
            rescore_touched<kMaxTouchedSlots, PRIO, DOM, LAB, F53>(cx, rc, rm, rp, sel, rcf, rmf, rpf, thk, thi, df, tk,
                                                                   ti, ts, any);
    }
    if (ST) { asm volatile("" ::"v"(tk), "v"(ti), "v"(ts)); t1 = stamp(); }
    if (any) wave_argbest_fast(tk, ti, ts);
    if (ST) { asm volatile("" ::"v"(tk), "v"(ti), "v"(ts)); t2 = stamp(); }
    const int64_t fc = ps.fc0 + df;
    int32_t oidx = -1;
    double osc = 0.0;
    int kind = 0;  // 0 none, 1 winner from list (new touch), 2 winner already touched, 3 overflow
    double wk = 0.0;
    int32_t wi = kNoIdx;
    if (fc != 0) {
        if (uq < cv) {
            const double uk = readlane_f64(my.key, uq);
            const int32_t ui = __builtin_amdgcn_readlane(my.idx, uq);
            if (ti != kNoIdx && better(tk, ti, uk, ui)) { kind = 2; wk = tk; wi = ti; }
            else { kind = 1; wk = uk; wi = ui; }
        } else if (!cut) {
            if (ti != kNoIdx) { kind = 2; wk = tk; wi = ti; }
        } else if (cv > 0) {
            const double lk = readlane_f64(my.key, cv - 1);
            const int32_t li = __builtin_amdgcn_readlane(my.idx, cv - 1);
            if (ti != kNoIdx && better(tk, ti, lk, li)) { kind = 2; wk = tk; wi = ti; }
            else kind = 3;
        } else {
            kind = 3;  // unreachable: a cut list keeps at least its cutoff entry
        }
    }
    if (ST) t3 = stamp();
    if (kind == 3) return true;  // overflow: stop before pod i (wave-uniform)
    if (fc != 0) {
        if (kind == 0) {
            oidx = -2;
        } else {
            oidx = wi;
            osc = PRIO == kPrioPrice ? 0.0 - wk : wk;
            ++cx.placed;
            int slot = ts;
            int writer = 0;
            int64_t b0, b1, b2;
            if (kind == 1) {  // first touch: the holder of the candidate opens the slot
                slot = cx.nT++;
                writer = uq;
                b0 = my.a[0]; b1 = my.a[1]; b2 = my.a[2];
                if (lane == uq) {
                    Touched &x = cx.T[slot];
                    x.idx = my.idx; x.mine = 1;
                    x.s0[0] = b0; x.s0[1] = b1; x.s0[2] = b2;
                    x.sb[0] = b0; x.sb[1] = b1; x.sb[2] = b2;  // untouched by the previous batch
                    x.labels = my.labels; x.price = my.price; x.pad2 = 0;
                    touched_insert(cx, my.idx);
                }
            } else {
                b0 = cx.T[slot].cur[0]; b1 = cx.T[slot].cur[1]; b2 = cx.T[slot].cur[2];
            }
            if (lane == writer) {
                Touched &x = cx.T[slot];
                x.mine = 1;
                const int64_t c0 = wsub(b0, rc), c1 = wsub(b1, rm), c2 = wsub(b2, 1);
                x.cur[0] = c0; x.cur[1] = c1; x.cur[2] = c2;
                x.curf[0] = (double)c0; x.curf[1] = (double)c1; x.curf[2] = (double)c2;
                x.cury[0] = recip_or_zero(c0, x.curf[0]);
                x.cury[1] = recip_or_zero(c1, x.curf[1]);
                x.cury[2] = recip_or_zero(c2, x.curf[2]);
            }
        }
    }
    if (lane == 0) {
        const int64_t pod = cx.p0 + i;
        A.out.idx[pod] = oidx;
        A.out.score[pod] = osc;
        A.out.feas[pod] = (int32_t)fc;
    }
    if (ST) {
        const uint64_t t4 = stamp();
        ph[0] += t1 - t0; ph[1] += t2 - t1; ph[2] += t3 - t2; ph[3] += t4 - t3;
    }
    return false;
}

template <int K, int PRIO, int DOM, bool LAB, bool F53, bool ST>
__device__ __forceinline__ int commit_loop(const CommitArgs &A, CommitCtx &cx, int nb, uint64_t *ph) {
    // pod i+1's staged request and candidates are read from LDS while pod i is being decided
    PodStage ps = cx.PS[0];
    CandStage my;
    if (cx.lane < K) my = cx.CS[cx.lane];
    else { my.idx = kNoIdx; my.key = -__builtin_inf(); }
    for (int i = 0; i < nb; ++i) {
        PodStage ps_n = ps;
        CandStage my_n = my;
        if (i + 1 < nb) {
            ps_n = cx.PS[i + 1];
            if (cx.lane < K) my_n = cx.CS[(i + 1) * K + cx.lane];
        }
        if (commit_step<K, PRIO, DOM, LAB, F53, ST>(A, cx, i, ps, my, ph)) return i;
        ps = ps_n;
        my = my_n;
    }
    return nb;
}

template <int K, int PRIO, int DOM, bool LAB, bool F53>
__global__ __launch_bounds__(64) void k_commit(CommitArgs A) {
    __builtin_amdgcn_s_setprio(3);  // latency-critical: win issue arbitration over co-resident score waves
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int64_t p0 = *A.plan;
    const int64_t cursor = A.ctl->cursor;
    if (p0 < 0 || p0 >= A.pods.p || p0 != cursor) {
        // nothing to do, or a speculative batch invalidated by an earlier truncation: skip it
        if (lane == 0) {
            A.xout->count = 0;
            if (p0 >= 0 && p0 < A.pods.p) A.ctl->stats[3] += 1;
            plan_after_commit(A, false, cursor);
        }
        publish_committed(A);
        return;
    }
    CommitCtx cx;
    cx.hkey = reinterpret_cast<int32_t *>(smem);
    char *p = smem + kTouchHash * sizeof(int32_t);
    cx.filt = reinterpret_cast<uint32_t *>(p);
    p += kTouchFilterWords * sizeof(uint32_t);
    cx.T = reinterpret_cast<Touched *>(p);
    p += (size_t)2 * A.B * sizeof(Touched);
    PodStage *PS = reinterpret_cast<PodStage *>(p);
    p += (size_t)A.B * sizeof(PodStage);
    CandStage *CS = reinterpret_cast<CandStage *>(p);
    cx.PS = PS;
    cx.CS = CS;
    cx.lane = lane;
    cx.placed = 0;
    cx.p0 = p0;
    const int nb = (int)((A.pods.p - p0 < A.B) ? A.pods.p - p0 : A.B);
    cx.y3 = recip(3.0);
    for (int w = lane; w < kTouchHash; w += 64) cx.hkey[w] = -1;
    for (int w = lane; w < kTouchFilterWords; w += 64) cx.filt[w] = 0;
    for (int b = lane; b < nb; b += 64) {
        PodStage s;
        s.rc = A.pods.rc[p0 + b]; s.rm = A.pods.rm[p0 + b]; s.rp = A.pods.rp[p0 + b];
        s.sel = LAB ? A.pods.sel[p0 + b] : 0;
        s.fc0 = A.fc0[b];
        s.cut = A.lists[(size_t)b * K].pad;
        s.pad = 0;
        PS[b] = s;
    }
    for (int e = lane; e < nb * K; e += 64) {
        const Rec r = A.lists[e];
        CandStage c;
        c.key = r.key; c.idx = r.valid ? r.idx : kNoIdx; c.price = r.price;
        c.a[0] = r.a[0]; c.a[1] = r.a[1]; c.a[2] = r.a[2]; c.labels = r.labels;
        CS[e] = c;
    }
    __syncthreads();
    // inherit the nodes the previous batch committed: this batch was scored before those commits
    const int nin = A.xin->count;
    for (int e = lane; e < nin; e += 64) {
        const XRec &xi = A.xin->e[e];
        Touched &x = cx.T[e];
        x.idx = xi.idx; x.mine = 0;
        for (int r = 0; r < 3; ++r) {
            x.s0[r] = xi.sb[r];
            x.sb[r] = xi.cur[r];
            x.cur[r] = xi.cur[r];
            x.curf[r] = (double)xi.cur[r];
            x.cury[r] = recip_or_zero(xi.cur[r], x.curf[r]);
        }
        x.labels = xi.labels; x.price = xi.price; x.pad2 = 0;
        uint32_t h = thash(xi.idx);
        while (atomicCAS(&cx.hkey[h], -1, xi.idx) != -1) h = (h + 1) & (kTouchHash - 1);
        atomicOr(&cx.filt[((uint32_t)xi.idx & 0xffffu) >> 5], 1u << ((uint32_t)xi.idx & 31));
    }
    cx.nT = nin;
    __syncthreads();

    uint64_t ph[4] = {0, 0, 0, 0};
    int done;
    if (A.dbg) {
        const uint64_t tl0 = stamp();
        done = commit_loop<K, PRIO, DOM, LAB, F53, true>(A, cx, nb, ph);
        const uint64_t tl1 = stamp();
        if (lane == 0) {
            A.dbg[0] += ph[0]; A.dbg[1] += ph[1]; A.dbg[2] += ph[2]; A.dbg[3] += ph[3];
            A.dbg[4] += tl1 - tl0; A.dbg[5] += done; A.dbg[6] += cx.nT; A.dbg[7] += 1;
        }
    } else {
        done = commit_loop<K, PRIO, DOM, LAB, F53, false>(A, cx, nb, ph);
    }
    __syncthreads();
    // export this batch's commits (wave-ordered compaction)
    int base = 0;
    for (int t0 = 0; t0 < cx.nT; t0 += 64) {
        const int t = t0 + lane;
        const bool m = t < cx.nT && cx.T[t].mine;
        const uint64_t mask = __ballot(m);
        if (m) {
            const Touched &x = cx.T[t];
            XRec &o = A.xout->e[base + __popcll(mask & ((1ull << lane) - 1))];
            o.idx = x.idx; o.pad = 0;
            o.sb[0] = x.sb[0]; o.sb[1] = x.sb[1]; o.sb[2] = x.sb[2];
            o.cur[0] = x.cur[0]; o.cur[1] = x.cur[1]; o.cur[2] = x.cur[2];
            o.labels = x.labels; o.price = x.price; o.pad2 = 0;
        }
        base += __popcll(mask);
    }
    if (lane == 0) {
        A.xout->count = base;
        A.ctl->cursor = p0 + done;
        A.ctl->stats[0] += 1;
        A.ctl->stats[1] += (done < nb) ? 1 : 0;
        A.ctl->stats[2] += cx.placed;
        plan_after_commit(A, done < nb, p0 + done);
    }
    publish_committed(A);
}

// Write one batch's committed nodes into this rank's node rows.
__global__ void k_apply_batch(const XBuf *x, NodeRec *nodes, int64_t node_lo, int64_t n_local) {
    const int n = x->count;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const XRec &r = x->e[e];
        const int64_t j = (int64_t)r.idx - node_lo;
        if (j >= 0 && j < n_local) set_node(nodes + j, r.cur[0], r.cur[1], r.cur[2]);
    }
}

// ---- launchers ----
namespace {
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a kernel on ONE device, and a context chooses its device
// (ksched_options::device): the (device ordinal, kernel) pairs that have it.  Contexts run on threads of their own.
std::mutex g_lds_mu;
std::set<std::pair<int, const void *>> g_lds_set;
}  // namespace

hipError_t launch_stream_kernel(const StreamKernel &k, dim3 grid, dim3 block, const void *arg, size_t lds,
                                hipStream_t s) {
    int dev = 0;
    hipError_t e = k.fn ? hipGetDevice(&dev) : hipErrorInvalidValue;
    if (e != hipSuccess) return e;
    {
        std::lock_guard<std::mutex> lk(g_lds_mu);
        if (!g_lds_set.count({dev, k.fn})) {
            e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
            if (e != hipSuccess) return e;
            g_lds_set.insert({dev, k.fn});
        }
    }
    void *args[] = {const_cast<void *>(arg)};
    return hipLaunchKernel(k.fn, grid, block, args, lds, s);
}

namespace {
template <int PRIO, int DOM, bool LAB, bool F53>
StreamKernel score_kc(int KC) {
    switch (KC) {
        case 2: return {(const void *)k_score_topk<2, PRIO, DOM, LAB, F53>, score_lds_bytes(2)};
        case 4: return {(const void *)k_score_topk<4, PRIO, DOM, LAB, F53>, score_lds_bytes(4)};
        case 8: return {(const void *)k_score_topk<8, PRIO, DOM, LAB, F53>, score_lds_bytes(8)};
        case 16: return {(const void *)k_score_topk<16, PRIO, DOM, LAB, F53>, score_lds_bytes(16)};
        default: return {};
    }
}
StreamKernel score_kernel(int KC, int prio, int dom, bool lab, bool f53) {
    KSCHED_DISPATCH(prio, dom, lab, f53, (score_kc<P_, D_, L_, F_>(KC)));
}

// k_commit's LDS depends on the batch (commit_lds_bytes(B, K), the launcher's argument): admitted up to the limit
constexpr size_t kSeqCommitMaxLds = 160 * 1024 - 4096;
template <int PRIO, int DOM, bool LAB, bool F53>
StreamKernel seq_commit_k(int K) {
    switch (K) {
        case 4: return {(const void *)k_commit<4, PRIO, DOM, LAB, F53>, kSeqCommitMaxLds};
        case 8: return {(const void *)k_commit<8, PRIO, DOM, LAB, F53>, kSeqCommitMaxLds};
        case 16: return {(const void *)k_commit<16, PRIO, DOM, LAB, F53>, kSeqCommitMaxLds};
        default: return {};
    }
}
StreamKernel seq_commit_kernel(int K, int prio, int dom, bool lab, bool f53) {
    KSCHED_DISPATCH(prio, dom, lab, f53, (seq_commit_k<P_, D_, L_, F_>(K)));
}
int alloc_vgprs(int n) { return (n + 7) / 8 * 8; }
}  // namespace

bool commit_fits_beside_score(int KC, int K, int B, bool spc, int prio, int dom, bool lab, bool f53) {
    hipFuncAttributes sa{}, ca{};
    const StreamKernel sk = score_kernel(KC, prio, dom, lab, f53);
    const StreamKernel ck = spc ? commit_spc_kernel(K, prio, dom, lab, f53) : seq_commit_kernel(K, prio, dom, lab, f53);
    if (!sk.fn || hipFuncGetAttributes(&sa, sk.fn) != hipSuccess) return false;
    if (!ck.fn || hipFuncGetAttributes(&ca, ck.fn) != hipSuccess) return false;
    const size_t commit_lds = spc ? ck.lds : commit_lds_bytes(B, K);
    const int score_waves_per_simd = kScoreThreads / 64 / 4;
    const int commit_waves_per_simd = spc ? kSpcThreads / 64 / 4 : 1;
    const int vgpr = score_waves_per_simd * alloc_vgprs(sa.numRegs) + commit_waves_per_simd * alloc_vgprs(ca.numRegs);
    const size_t lds = sa.sharedSizeBytes + sk.lds + ca.sharedSizeBytes + commit_lds;
    const int waves = kScoreThreads / 64 + (spc ? kSpcThreads / 64 : 1);
    return vgpr <= 512 && lds <= 160 * 1024 && waves <= 32;
}

hipError_t launch_score_topk(int KC, int prio, int dom, bool lab, bool f53, const ScoreArgs &a, int pod_groups,
                             hipStream_t s) {
    const StreamKernel k = score_kernel(KC, prio, dom, lab, f53);
    return launch_stream_kernel(k, dim3((unsigned)(a.n_chunks / kScoreWaves), pod_groups), dim3(kScoreThreads), &a,
                                k.lds, s);
}

hipError_t launch_commit(int K, int prio, int dom, bool lab, bool f53, const CommitArgs &a, size_t lds_bytes,
                         hipStream_t s) {
    return launch_stream_kernel(seq_commit_kernel(K, prio, dom, lab, f53), dim3(1), dim3(64), &a, lds_bytes, s);
}

namespace {
template <int K>
hipError_t merge_pod_k(int KC, const MergeArgs &a, hipStream_t s) {
    switch (KC) {
        case 2: hipLaunchKernelGGL((k_merge_pod<2, K>), dim3(a.B), dim3(kMergeThreads), 0, s, a); break;
        case 4: hipLaunchKernelGGL((k_merge_pod<4, K>), dim3(a.B), dim3(kMergeThreads), 0, s, a); break;
        case 8: hipLaunchKernelGGL((k_merge_pod<8, K>), dim3(a.B), dim3(kMergeThreads), 0, s, a); break;
        case 16: hipLaunchKernelGGL((k_merge_pod<16, K>), dim3(a.B), dim3(kMergeThreads), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int K>
hipError_t rank_merge_k(const MergeArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_merge<K>), dim3(a.C_out, a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_merge_pod(int KC, int K, const MergeArgs &a, hipStream_t s) {
    if (a.C_in > kMergeThreads || KC > K) return hipErrorInvalidValue;
    switch (K) {
        case 4: return merge_pod_k<4>(KC, a, s);
        case 8: return merge_pod_k<8>(KC, a, s);
        case 16: return merge_pod_k<16>(KC, a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rank_merge(int K, const MergeArgs &a, hipStream_t s) {
    switch (K) {
        case 4: return rank_merge_k<4>(a, s);
        case 8: return rank_merge_k<8>(a, s);
        case 16: return rank_merge_k<16>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_apply_batch(const XBuf *x, NodeRec *nodes, int64_t node_lo, int64_t n_local, hipStream_t s) {
    hipLaunchKernelGGL(k_apply_batch, dim3(1), dim3(256), 0, s, x, nodes, node_lo, n_local);
    return hipGetLastError();
}

}  // namespace ksched
