// unique_id_kernels.hpp -- launcher of unique_id_kernels.hip: the id column of AssignUniqueIdOperator.
//
// The ids of a page are a few arithmetic runs: rows take consecutive row ids out of the operator's current block of the pool, and where
// the block is used up in the middle of a page the next row starts the next block (AssignUniqueIdOperator.java:142-161).  The host
// knows where the blocks end, so it hands the device the runs -- (first row, rows, first id) -- and the kernel only writes: one
// 8-byte store per row, one writer per element, nothing read.
#pragma once

#include "common.hpp"

namespace pa {

constexpr int kUniqueIdSegments = 8;   // runs of one launch: a page of up to 7 * 2^20 rows; a longer page takes further launches

struct UniqueIdArgs {
    int64_t* ids;                          // out, by position of the page
    int32_t first_row[kUniqueIdSegments];  // ascending; segment k covers [first_row[k], first_row[k] + rows[k])
    int32_t rows[kUniqueIdSegments];
    int64_t first_id[kUniqueIdSegments];   // the id of the segment's first row, mask included
    int32_t segments;                      // 1 .. kUniqueIdSegments, one behind the other without a gap
    int32_t pad;
};
// ids[first_row[k] + j] = first_id[k] + j for every segment k and j < rows[k]
void launch_unique_ids(const UniqueIdArgs& a, hipStream_t s);

}  // namespace pa
