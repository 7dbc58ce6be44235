// ksched_rank.h -- ksched_rank's two kernels (ksched_rank.hip) as the host sees them: the geometry, the
// workspace layout and the launcher.  Dry run: nothing here writes a node row.
#pragma once

#include "ksched_kernels.h"

namespace ksched {

constexpr int kRankList = 64;     // entries kept per pod: one per lane (= KSCHED_RANK_MAX)
constexpr int kRankWaves = 4;     // waves of a scan (and of a merge) workgroup
constexpr int kRankThreads = kRankWaves * 64;
constexpr int kRankTile = 8;      // pods a scan wave carries: 3 VGPRs of list each
constexpr int kRankInsertMax = 8;  // rows of a step beating the bar: up to here inserted singly, above sorted and merged
constexpr int kRankSpanMin = 1024;   // node rows of the shortest span: 4 steps of the workgroup's 256 lanes
constexpr int kRankGridWGs = 2048;   // spans x pod tiles a scan launch aims at (8 workgroups per CU)
constexpr int kRankChunk = 1024;     // pods per pair of launches: the workspace holds one chunk

struct RankArgs {
    const NodeRec *nodes;  // read only
    int64_t n_local, node_offset;
    const int64_t *rc, *rm, *rp;  // the chunk's pods (device)
    const uint64_t *sel;
    int32_t m;             // pods in the chunk (<= kRankChunk)
    int32_t spans;         // node spans (scan grid x)
    int64_t span_rows;     // rows per span, a multiple of kRankThreads
    Cand *part;            // [m][spans][kRankList], best first, idx = kNoIdx past the end
    int32_t *part_fc;      // [m][spans] nodes of the span passing the predicate
    int32_t k;             // entries wanted (1..kRankList)
    int32_t *out_idx;      // [m][k]
    double *out_score;     // [m][k]
    uint8_t *out_reason;   // [m][k]
    int32_t *out_count;    // [m]
    int32_t *out_feasible; // [m]
};

// The spans of a chunk of m pods over n rows: as many as keep the scan grid near kRankGridWGs workgroups, none
// shorter than kRankSpanMin rows.  m = 1 .. 8: ceil(n / 1024) spans (at most 2048); a full chunk: at most 16.
// spans * m <= kRankGridWGs * kRankTile lists of 1 KiB: the part lists never exceed 16 MiB.
// (tile: the pods a scan wave carries -- ksched_dryrun.hip's scan has the same geometry at a smaller tile)
inline void rank_geometry(int64_t n, int64_t m, int32_t *spans, int64_t *span_rows, int tile = kRankTile) {
    const int64_t tiles = (m + tile - 1) / tile;
    int64_t s = kRankGridWGs / (tiles < 1 ? 1 : tiles);
    const int64_t smax = (n + kRankSpanMin - 1) / kRankSpanMin;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    int64_t rows = (n + s - 1) / s;
    rows = (rows + kRankThreads - 1) / kRankThreads * kRankThreads;
    if (rows < kRankThreads) rows = kRankThreads;
    *span_rows = rows;
    *spans = (int32_t)((n + rows - 1) / rows < 1 ? 1 : (n + rows - 1) / rows);
}

// k_rank_scan then k_rank_merge on s: two ordinary launches, no waits on the device
hipError_t launch_rank(int prio, int dom, bool lab, bool fast53, const RankArgs &a, hipStream_t s);

}  // namespace ksched
