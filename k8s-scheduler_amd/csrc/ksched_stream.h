// ksched_stream.h -- the interface of the stream pipeline (ksched_stream.hip, ksched_commit_spc.hip; DESIGN.md section
// 4.3): batched mode as one launch per stage and batch, for enqueue_batched (ksched_engine.hip):
//   k_score_topk   pod-per-lane fused predicate + score + per-lane top-KC over a node chunk (scalar row loads);
//   k_merge_pod    one workgroup per pod: the score workgroups' lists -> the pod's K-entry Rec list;
//   k_merge        R > 1: sorted-list merge of the ranks' lists, one wave per pod, DPP/shuffle arg-best;
//   k_commit       one wave replays the batch in pod order: re-scores the nodes already committed in the batch,
//                  takes the first untouched candidate, commits, stops at the first candidate-list overflow;
//   k_commit_spc   the same decisions by speculation and a parallel check (commit_spc_batch, ksched_commit.h), B <= 64;
//   k_apply_batch  a call's last commits into the node rows.
#pragma once

#include "ksched_kernels.h"

namespace ksched {

struct ScoreArgs {
    NodeRec *nodes;    // read; the rows of `patch` are written back by their chunk's wave
    int64_t n_local;
    int64_t node_offset;
    int32_t S;         // unused
    int32_t n_chunks;  // NSC sub-chunks = workgroups x kScoreWaves
    PodArgs pods;
    const int64_t *cursor;  // this batch's plan slot (first pod, or -1)
    int32_t B;
    Cand *part;        // [B][workgroups][KC]
    int64_t *part_cnt; // [B][workgroups]
    const XBuf *patch; // batch b-2's commits: overlaid on the rows as they are read, then written back
    // device-side wait for commit(b-2): poll *wait_committed >= wait_target (null: the stream waits)
    const unsigned long long *wait_committed;
    unsigned long long wait_target;
    int32_t *err;                    // device error word (kErrStreamScoreWait)
};

// score kernel geometry: kScoreWaves waves per workgroup
constexpr int kScoreWaves = 8;
constexpr int kMergeThreads = 512;  // merge: one workgroup per pod, lane = one workgroup list (<= 512)
constexpr int kScoreThreads = kScoreWaves * 64;
constexpr size_t score_lds_bytes(int KC) { return (size_t)(kScoreWaves / 2) * KC * 64 * 12 + 64 * 4; }

// k_commit's touched-node table: a node it committed to, or inherited from the previous batch's export
struct alignas(8) Touched {
    int32_t idx;
    int32_t mine;     // committed to by a pod of THIS batch (exported to the next batch)
    int64_t s0[3];    // state at this batch's score snapshot
    int64_t sb[3];    // state when this batch's commit started
    int64_t cur[3];   // current state
    double curf[3];   // (double)cur
    double cury[3];   // recip((double)cur)
    uint64_t labels;
    float price;
    int32_t pad2;
};
static_assert(sizeof(Touched) == 144, "Touched layout");

struct alignas(8) PodStage {
    int64_t rc, rm, rp;
    uint64_t sel;
    int64_t fc0;
    int32_t cut;  // the pod's merged list is cut (entry 0's pad; see k_merge)
    int32_t pad;
};

// A candidate as staged in the commit kernel's LDS (idx = kNoIdx for an empty slot).
struct alignas(8) CandStage {
    double key;
    int32_t idx;
    float price;
    int64_t a[3];
    uint64_t labels;
};
static_assert(sizeof(CandStage) == 48, "CandStage layout");

constexpr int kTouchHashBits = 9;  // touched-node set: 512 slots >= 2 x max batch (256)
constexpr int kTouchHash = 1 << kTouchHashBits;
constexpr int kTouchFilterBits = 16;  // 64K-bit filter in front of the hash (bit = idx & 0xffff)
constexpr int kTouchFilterWords = (1 << kTouchFilterBits) / 32;

// LDS bytes of k_commit for a batch of B pods with K candidates each (touched table: the previous
// batch's nodes + this batch's, <= 2B).
constexpr size_t commit_lds_bytes(int B, int K) {
    return kTouchHash * sizeof(int32_t) + kTouchFilterWords * sizeof(uint32_t) +
           (size_t)B * (2 * sizeof(Touched) + sizeof(PodStage) + (size_t)K * sizeof(CandStage));
}

constexpr size_t xbuf_bytes(int B) { return 16 + (size_t)2 * B * sizeof(XRec); }

// host-side launchers.  fast53: every allocatable and request magnitude stays below 2^52 for the whole call
// (host-checked), enabling (double)(a-r) == (double)a - (double)r.
hipError_t launch_score_topk(int KC, int prio, int dom, bool lab, bool fast53, const ScoreArgs &a, int pod_groups,
                             hipStream_t s);
// one workgroup per pod: the score kernel's workgroup lists -> the pod's K-entry Rec list (C_in <= 512)
hipError_t launch_merge_pod(int KC, int K, const MergeArgs &a, hipStream_t s);
// one wave per pod: the ranks' K-entry Rec lists (the all-gather layout) -> the pod's global K-entry Rec list
hipError_t launch_rank_merge(int K, const MergeArgs &a, hipStream_t s);
hipError_t launch_commit(int K, int prio, int dom, bool lab, bool fast53, const CommitArgs &a, size_t lds_bytes,
                         hipStream_t s);
hipError_t launch_commit_spc(int K, int prio, int dom, bool lab, bool fast53, const CommitArgs &a, hipStream_t s);
hipError_t launch_apply_batch(const XBuf *x, NodeRec *nodes, int64_t node_lo, int64_t n_local, hipStream_t s);
// Can the batch's commit workgroup dispatch onto a CU that holds a score workgroup (VGPRs, LDS, wave
// slots)?  Only then may score(b) be resident and poll for commit(b-2): otherwise the score grid
// could occupy every CU while the commit it waits for never gets in.
bool commit_fits_beside_score(int KC, int K, int B, bool spc, int prio, int dom, bool lab, bool fast53);

// One instantiation of k_score_topk, k_commit or k_commit_spc, as its variant lookup resolves the runtime
// parameters (fn null: none for that KC / K).  Launcher and attribute query both start from it.
struct StreamKernel {
    const void *fn = nullptr;
    size_t lds = 0;  // dynamic LDS the kernel is admitted to (score, spc: the bytes it is launched with)
};
StreamKernel commit_spc_kernel(int K, int prio, int dom, bool lab, bool fast53);  // ksched_commit_spc.hip
// k with its one argument struct and `lds` <= k.lds bytes of dynamic LDS; the first launch of k on a device sets
// hipFuncAttributeMaxDynamicSharedMemorySize = k.lds there
hipError_t launch_stream_kernel(const StreamKernel &k, dim3 grid, dim3 block, const void *arg, size_t lds,
                                hipStream_t s);

}  // namespace ksched
