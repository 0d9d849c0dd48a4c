// topn_ranking_kernels.hpp -- launchers of topn_ranking_kernels.hip: the passes of TopNRankingOperator (op_topn_ranking.cpp).
//
// Per page (the hot path): every row has a group id (distinct_kernels.hpp) and the order-preserving image of its first sort channel
// (topn_kernels.hpp: monotone, not injective, NULL placement folded in).  bound[gid] is the image of the partition's current n-th row,
// ~0 while the partition holds fewer than n rows.  A row with image > bound[gid] can never be kept; a row with image == bound[gid] may
// still win or tie on a later sort channel, so it survives to the exact comparison.
//
// Per prune: the held rows are sorted by (gid, sort channels) with arrival order inside ties (row_sort.hpp); the passes here turn the
// sorted order into row numbers / ranks, keep flags and the new bounds:
//   heads:  the first row of each gid run stores its index in run_start[gid]; for RANK the first row of each peer run (a gid head, or a
//           row that differs from its predecessor on some sort channel) is flagged, and an exclusive scan of the flags numbers the
//           peer runs;
//   peers:  the head of peer run p stores its index in peer_start[p];
//   rank:   rn = i - run_start[gid] + 1, rank = peer_start[p] - run_start[gid] + 1; keep = value <= n; the row that stands at place n
//           of its run writes bound[gid].
// Every array element has one writer and no pass reads what the same launch writes: nothing depends on the order in which waves run.
#pragma once

#include "common.hpp"

namespace pa {

constexpr int kTopNRankingRowsPerBlock = 1024;   // rows of one workgroup of the arrival filter: 256 lanes x 4

// keep[i] = images[i] <= bound[gids[i]] (ids not below bound_n: partitions first seen after the last prune, bound ~0).  keep:
// round_up(n, 4) bytes, the layout launch_row_number_keep_counts reads.
void launch_topn_ranking_filter(const uint64_t* gids, const uint64_t* images, const uint64_t* bound, int64_t bound_n, int32_t n, uint8_t* keep,
                                hipStream_t s);

// differs[i] |= row perm[i] and row perm[i - 1] are not equal on this sort channel (both NULL = equal; DOUBLE / REAL: any NaN equals any
// NaN, -0.0 differs from +0.0 -- the comparator's equality; VARCHAR: length and bytes; BOOLEAN: zero / non-zero)
void launch_topn_ranking_differs(int32_t type, const void* values, const int32_t* offsets, const uint8_t* nulls, const int32_t* perm, int32_t n,
                                 uint8_t* differs, hipStream_t s);

// run_start[gid] = index of the first row of the gid's run (ids below run_start_n); peer_flag (may be null; n entries): 1 at the first
// row of each peer run.  differs may be null only when peer_flag is.
void launch_topn_ranking_heads(const uint64_t* sorted_gids, const uint8_t* differs, int32_t n, int32_t* run_start, int64_t run_start_n, int32_t* peer_flag,
                               hipStream_t s);
// peer_start[peer_index[i]] = i for every flagged i (peer_index = exclusive scan of peer_flag)
void launch_topn_ranking_peer_starts(const int32_t* peer_flag, const int32_t* peer_index, int32_t n, int32_t* peer_start, hipStream_t s);

struct TopNRankingRankArgs {
    const uint64_t* sorted_gids;   // n, ascending
    const int32_t* perm;           // sorted index -> held row
    const uint64_t* images;        // by held row: first sort channel's image, as the arrival filter sees it
    const int32_t* run_start;      // by gid
    int64_t run_start_n;
    const int32_t* peer_flag;      // RANK only, else null
    const int32_t* peer_index;
    const int32_t* peer_start;
    int64_t limit;                 // maxRowCountPerPartition
    uint64_t* bound;               // by gid: written by the row at place `limit` of its run
    int64_t bound_n;
    int64_t* ranking;              // out, by sorted index: row number / rank
    uint8_t* keep;                 // out, by sorted index: ranking <= limit
    int32_t n;
    int32_t pad;
};
void launch_topn_ranking_rank(const TopNRankingRankArgs& a, hipStream_t s);

}  // namespace pa
