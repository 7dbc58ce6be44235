// ksched_preempt.h -- ksched_preempt's two kernels (ksched_preempt.hip) and the bound-pod table they read, as the
// host sees them: the table's layout, the geometry, the workspace and the launcher.  Dry run: nothing here writes a
// node row.
#pragma once

#include <vector>

#include "ksched_kernels.h"

namespace ksched {

constexpr int kPreemptWaves = 4;     // waves of a scan workgroup: 256 consecutive nodes per step
constexpr int kPreemptThreads = kPreemptWaves * 64;
constexpr int kPreemptTile = 4;      // pods a scan wave carries (wave-uniform requests, 13 VGPRs of state each): 87 VGPRs,
                                     // 5 waves per SIMD.  Measured against 8 (140 VGPRs, 3 waves, twice the SGPR spills):
                                     // 6.0 against 7.25 ms for 1024 pods on c4's table
constexpr int kPreemptSpanMin = 1024;  // node rows of the shortest span
constexpr int kPreemptGridWGs = 2048;  // spans x pod tiles a scan launch aims at (8 workgroups per CU)
constexpr int kPreemptChunk = 1024;    // pods per pair of launches: the workspace holds one chunk
constexpr int kBoundMaxPerNode = 1024; // KSCHED_BOUND_MAX_PER_NODE
constexpr int kPreemptCntBits = 11;    // a node's victim count (<= 1024) in the low bits of PreemptPart::sc

// The bound-pod table on the device.  Nodes are taken in blocks of 64 consecutive (local) nodes, block b = nodes
// [64 b, 64 b + 64); a node's pods are its SEGMENT, ordered by ascending importance (prio ascending, then table index
// descending), so the potential victims of any preemptor are a prefix of it.  A block is stored slot-major:
//   entry (block b, slot s, lane l) = column[off[b] + s * 64 + l],   0 <= s < depth[b] = the block's longest segment
// so a wave with lane = node reads slot s of its 64 nodes in one coalesced access per column.  Slots past a node's
// own segment (and the lanes past the last node) are padding: cpu = mem = 0, prio = INT32_MAX (below no preemptor's
// priority: padding never takes part), tidx = -1.
struct BoundTable {
    const int64_t *cpu, *mem;  // [entries]
    const int32_t *prio;       // [entries]
    const int32_t *tidx;       // [entries] the pod's index in the caller's table
    const int64_t *off;        // [blocks] first entry of the block
    const int32_t *depth;      // [blocks]
    const int32_t *seg;        // [n_local] the node's own segment length
};

// The host side of the build (ksched_data.hip: build_bound_table).  entries = 64 * sum of depth.
struct BoundTableHost {
    std::vector<int64_t> cpu, mem, off;
    std::vector<int32_t> prio, tidx, depth, seg;
};
// Counting sort by node, each segment by ascending importance, laid out as above.  false: a node index outside
// [0, n), or a segment above kBoundMaxPerNode (*why names which).  Host only; throws std::bad_alloc.
bool build_bound_table(int64_t n, int64_t nb, const int32_t *node_idx, const int64_t *cpu, const int64_t *mem,
                       const int32_t *prio, BoundTableHost *out, const char **why);

// A node's key for one preemptor, smaller is better: mx = the largest victim priority + 2^31 (0: no victim), sc =
// (sum of (prio + 2^31) over the victims) << kPreemptCntBits | victim count -- at most 1024 victims of 32 bits each,
// so the sum stays below 2^42 and (sum, count) compare as one 53-bit number -- then the global node index.
// No candidate: (~0, ~0, kNoIdx).
struct alignas(16) PreemptPart {
    uint32_t mx;
    int32_t idx;
    uint64_t sc;
};
static_assert(sizeof(PreemptPart) == 16, "PreemptPart layout");

struct PreemptArgs {
    const NodeRec *nodes;  // read only
    int64_t n_local, node_offset;
    BoundTable tb;
    const int64_t *rc, *rm, *rp;  // the chunk's pods (device)
    const uint64_t *sel;
    const int32_t *prio;
    int32_t m;             // pods in the chunk (<= kPreemptChunk)
    int32_t spans;         // node spans (scan grid x)
    int64_t span_rows;     // rows per span, a multiple of kPreemptThreads
    PreemptPart *part;     // [m][spans] the span's best node
    int32_t *part_nc;      // [m][spans] candidate nodes of the span
    int32_t vcap;
    int32_t *out_node, *out_nvictims, *out_max_prio, *out_candidates;  // [m]
    int64_t *out_sum_prio;                                             // [m]
    int32_t *out_victims;                                              // [m][vcap]
};

// The spans of a chunk of m pods over n rows (rank_geometry's rule): as many as keep the scan grid near
// kPreemptGridWGs workgroups, none shorter than kPreemptSpanMin rows; spans * m <= kPreemptGridWGs * tile (tile: the
// scan's pods per wave).
inline void preempt_geometry(int64_t n, int64_t m, int32_t *spans, int64_t *span_rows, int tile = kPreemptTile) {
    const int64_t tiles = (m + tile - 1) / tile;
    int64_t s = kPreemptGridWGs / (tiles < 1 ? 1 : tiles);
    const int64_t smax = (n + kPreemptSpanMin - 1) / kPreemptSpanMin;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    int64_t rows = (n + s - 1) / s;
    rows = (rows + kPreemptThreads - 1) / kPreemptThreads * kPreemptThreads;
    if (rows < kPreemptThreads) rows = kPreemptThreads;
    *span_rows = rows;
    *spans = (int32_t)((n + rows - 1) / rows < 1 ? 1 : (n + rows - 1) / rows);
}

// k_preempt_scan then k_preempt_pick on s: two ordinary launches, no waits on the device
hipError_t launch_preempt(bool lab, const PreemptArgs &a, hipStream_t s);

}  // namespace ksched
