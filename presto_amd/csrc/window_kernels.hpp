// window_kernels.hpp -- launchers of window_kernels.hip: the passes of WindowOperator (op_window.cpp) behind its sort.
//
// The rows stand sorted by (partition channels, sort channels) as a permutation (row_sort.hpp).  By sorted index i:
//   flags     part_flag[i] / peer_flag[i] = 1 when i > 0 and sorted row i IS DISTINCT FROM sorted row i - 1 on a partition channel /
//             on a partition or a sort channel; one launch per channel ORs into the flags.  Row 0 is never flagged: it opens run 0.
//   scans     part_index / peer_index = exclusive scans of the flags (scan_kernels.hpp), so that the run of row i is
//             index[i] + flag[i]: the flags up to and including its own.
//   starts    the first row of run r stores its index in start[r]; row n - 1 also stores the sentinel n behind the last run.
//   functions per row: its partition p and peer group q, part_start[p], part_start[p + 1], peer_start[q], peer_start[q + 1] and the
//             peer group of part_start[p]; every requested column written by sorted index.
// Every array element has one writer per launch and no pass reads what the same launch writes: nothing is carried between workgroups
// and nothing depends on the order in which waves run.  Algorithmic bytes per row: flags 4 (perm) + two random rows per channel,
// scans 2 x (4 + 4), starts 16, functions 16 + 8 per column (+ 4 + the argument through perm for ntile); the start arrays are read at
// indices that never decrease with i.
#pragma once

#include "common.hpp"

namespace pa {

constexpr int kWindowRowsPerBlock = 1024;   // rows of one workgroup of the function pass: 256 lanes x 4
constexpr int kWindowMaxFunctions = 16;

// flag_a[i] = 1 (and flag_b[i] = 1 when flag_b is not null) for every 0 < i < n whose row perm[i] IS DISTINCT FROM row perm[i - 1] in
// this channel: both NULL = equal; DOUBLE / REAL: any NaN equals any NaN, -0.0 equals +0.0; VARCHAR: length and bytes; BOOLEAN:
// zero / non-zero; a short DECIMAL as its 8-byte value.  The flags are only ever set: the caller zeroes them before the first channel.
void launch_window_distinct(int32_t type, const void* values, const int32_t* offsets, const uint8_t* nulls, const int32_t* perm, int32_t n,
                            int32_t* flag_a, int32_t* flag_b, hipStream_t s);

// part_start[part_index[i] + part_flag[i]] = i for i = 0 and every flagged i, part_start[runs] = n; the same for the peer groups.
// part_start / peer_start: n + 1 entries.
void launch_window_starts(const int32_t* part_flag, const int32_t* part_index, const int32_t* peer_flag, const int32_t* peer_index, int32_t n,
                          int32_t* part_start, int32_t* peer_start, hipStream_t s);

struct WindowFunction {
    int32_t function;          // pa_window_function
    int32_t arg_type;          // ntile: PA_BIGINT / PA_INTEGER
    const void* arg_values;    // ntile: the argument channel by held row
    const uint8_t* arg_nulls;  // may be null
    void* out;                 // n x 8 bytes by sorted index: BIGINT, or DOUBLE for percent_rank / cume_dist
    uint8_t* out_nulls;        // ntile with arg_nulls: n bytes; else null
};
struct WindowFunctionArgs {
    const int32_t* perm;       // sorted index -> held row (read for ntile only)
    const int32_t* part_flag;
    const int32_t* part_index;
    const int32_t* peer_flag;
    const int32_t* peer_index;
    const int32_t* part_start;
    const int32_t* peer_start;
    int32_t* error;            // set to 1 by a row whose ntile bucket count is <= 0
    int32_t n;
    int32_t count;
    WindowFunction f[kWindowMaxFunctions];
};
void launch_window_functions(const WindowFunctionArgs& a, hipStream_t s);

}  // namespace pa
