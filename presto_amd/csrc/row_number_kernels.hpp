// row_number_kernels.hpp -- launchers of row_number_kernels.hip: the passes of RowNumberOperator behind the key table.
//
// Per page, every row has a group id (distinct_kernels.hpp: launch_distinct_group_ids) and needs
//   rn[i] = counts[gid[i]] + (rows j < i of the page with gid[j] == gid[i]) + 1          (RowNumberOperator.java:301-342)
// with counts carried from page to page.  The (gid, position) pairs are sorted by gid with the stable launch_sort_pairs, so that every
// group is one run in which positions ascend; the rank of a row inside the page is then its distance from the head of its run.
//
// Nothing here depends on the order in which waves run:
//   * the rank pass only READS counts; a workgroup takes kRowNumberRowsPerBlock consecutive pairs of the sorted order, finds the run
//     heads among them with a max-scan of head indices, and learns where the run that reaches into it from the left begins by a
//     search of its own in the sorted ids (gallop back, then bisect: equal ids are contiguous) -- there is no carry that one
//     workgroup hands to another, so no workgroup waits for, or races with, another;
//   * the last pair of each run leaves the run's new count in tails[] at its own index, and the update pass -- a launch of its own,
//     behind the rank pass -- stores it: one writer per group per page, no atomics.
#pragma once

#include "common.hpp"

namespace pa {

constexpr int kRowNumberRowsPerBlock = 1024;   // pairs of one workgroup of the rank pass, rows of one of the keep passes: 256 lanes x 4
inline int64_t row_number_blocks(int64_t n) { return (n + kRowNumberRowsPerBlock - 1) / kRowNumberRowsPerBlock; }

struct RowNumberRankArgs {
    const uint64_t* gids;     // sorted group ids (n)
    const int32_t* rows;      // the position in the page of each sorted pair (n)
    const int64_t* counts;    // rows numbered so far, by group id
    int64_t counts_n;         // entries of counts: a pair whose id is not below it is left alone (cannot happen unless the table failed)
    int64_t cap;              // maxRowsPerPartition, or -1
    int64_t* rn;              // out, by position: the row number
    uint8_t* keep;            // out, by position (cap >= 0 only): rn <= cap
    int64_t* tails;           // out, by sorted index: written for the last pair of a run only = counts[gid] + the run's length
    int32_t n;
    int32_t pad;
};
void launch_row_number_rank(const RowNumberRankArgs& a, hipStream_t s);
// counts[gid] = tails[j] (at most cap) for the last pair j of each run
void launch_row_number_update(const uint64_t* gids, const int64_t* tails, int32_t n, int64_t cap, int64_t* counts, int64_t counts_n, hipStream_t s);

// no partition channels: rn[i] = start + i + 1
void launch_row_number_iota(int64_t start, int32_t n, int64_t* rn, hipStream_t s);
// positions[i] = i (the kept prefix of a page of the single partition)
void launch_row_number_positions_iota(int32_t n, int32_t* positions, hipStream_t s);

// The rows kept under the cap, compacted in input order: keep (round_up(n, 4) bytes, the n first written) -> rows kept per block of
// kRowNumberRowsPerBlock rows -> [exclusive scan by the caller] -> positions
void launch_row_number_keep_counts(const uint8_t* keep, int32_t n, int32_t* block_counts, hipStream_t s);
void launch_row_number_keep_positions(const uint8_t* keep, int32_t n, const int32_t* block_offsets, int32_t* positions, hipStream_t s);

}  // namespace pa
