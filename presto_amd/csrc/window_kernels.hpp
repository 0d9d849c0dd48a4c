// window_kernels.hpp -- launchers of window_kernels.hip: the passes of WindowOperator (op_window.cpp) behind its sort.
//
// The rows stand sorted by (partition channels, sort channels) as a permutation (row_sort.hpp).  By sorted index i:
//   flags     part_flag[i] / peer_flag[i] = 1 when i > 0 and sorted row i IS DISTINCT FROM sorted row i - 1 on a partition channel /
//             on a partition or a sort channel; one launch per channel ORs into the flags.  Row 0 is never flagged: it opens run 0.
//   scans     part_index / peer_index = exclusive scans of the flags (scan_kernels.hpp), so that the run of row i is
//             index[i] + flag[i]: the flags up to and including its own.
//   starts    the first row of run r stores its index in start[r]; row n - 1 also stores the sentinel n behind the last run.
//   gather    (aggregates) per distinct argument channel: its values, widened to 8 bytes, and its NULL flags through perm into sorted
//             order; one gather serves every function on the channel.
//   agg scans (aggregates) per distinct (kind, channel): a segmented inclusive scan over sorted index that restarts where part_flag is
//             set -- tile aggregates, the scan of the tile aggregates, apply: three launches, as scan_kernels.hip scans.
//   functions per row: its partition p and peer group q, part_start[p], part_start[p + 1], peer_start[q], peer_start[q + 1] and the
//             peer group of part_start[p]; every requested column written by sorted index.  An aggregate column reads the scanned state
//             at the last row of its frame: part_start[p] + e, an index that never decreases with i.  A value column (lag, lead,
//             first_value, last_value, nth_value) copies the value channel's bytes, at the type's own width, from the held row
//             perm[part_start[p] + target]: not through the aggregates' gather, which holds 8 bytes and widens REAL.
// Every array element has one writer per launch and no pass reads what the same launch writes: nothing is carried between workgroups
// and nothing depends on the order in which waves run.  Algorithmic bytes per row: flags 4 (perm) + two random rows per channel,
// scans 2 x (4 + 4), starts 16, functions 16 + 8 per column (+ 4 + the argument through perm for ntile); the start arrays are read at
// indices that never decrease with i.  Aggregates: gather 4 (perm) + a random value (and NULL byte) + 8 (+ 1) written; a scan reads its
// input and part_flag twice (8 + 4 (+ 1) each time) and writes 8 (sum, min, max) or 4 (the non-null count); the function pass reads
// 8 (+ 4 with NULLs) more per aggregate column.  Value functions, per column: 4 (perm at the target: one entry per partition for
// first_value, a shifted run for lag / lead with a constant offset) + one random value of the type's width (+ its NULL byte) read, the
// width (+ 1) written; with an offset or default channel 4 more (perm at the row itself) + the random offset (4 / 8 (+ 1)) and, where
// the target leaves the partition, the random default.
#pragma once

#include "common.hpp"

namespace pa {

constexpr int kWindowRowsPerBlock = 1024;   // rows of one workgroup of the function pass: 256 lanes x 4
constexpr int kWindowMaxFunctions = 16;
constexpr int kWindowScanTile = 1024;       // rows of one workgroup of the aggregate scans: 256 lanes x 4 consecutive rows

// flag_a[i] = 1 (and flag_b[i] = 1 when flag_b is not null) for every 0 < i < n whose row perm[i] IS DISTINCT FROM row perm[i - 1] in
// this channel: both NULL = equal; DOUBLE / REAL: any NaN equals any NaN, -0.0 equals +0.0; VARCHAR: length and bytes; BOOLEAN:
// zero / non-zero; a short DECIMAL as its 8-byte value.  The flags are only ever set: the caller zeroes them before the first channel.
void launch_window_distinct(int32_t type, const void* values, const int32_t* offsets, const uint8_t* nulls, const int32_t* perm, int32_t n,
                            int32_t* flag_a, int32_t* flag_b, hipStream_t s);

// part_start[part_index[i] + part_flag[i]] = i for i = 0 and every flagged i, part_start[runs] = n; the same for the peer groups.
// part_start / peer_start: n + 1 entries.
void launch_window_starts(const int32_t* part_flag, const int32_t* part_index, const int32_t* peer_flag, const int32_t* peer_index, int32_t n,
                          int32_t* part_start, int32_t* peer_start, hipStream_t s);

// The argument channel of the aggregates in sorted order: sorted_values[i] = the value of row perm[i] as 8 bytes (BIGINT / short DECIMAL
// as they are, INTEGER / DATE sign-extended, BOOLEAN 0 / 1, DOUBLE its bits, REAL widened to a double's bits: exact), sorted_nulls[i] =
// its NULL flag.  Either output may be null (count reads the flags only; a channel without NULLs has none).
void launch_window_gather(int32_t type, const void* values, const uint8_t* nulls, const int32_t* perm, int32_t n, uint64_t* sorted_values,
                          uint8_t* sorted_nulls, hipStream_t s);

// The segmented inclusive scans of the aggregates over sorted index, restarting where part_flag is set.  A NULL row (sorted_nulls, may
// be null) leaves the state as it is.
enum WindowScanKind {
    kWindowScanCount = 0,   // out: int32 per row, the non-null rows of its partition up to and including it
    kWindowScanSum = 1,     // out: int64 per row, the sum of those rows' values; a row whose sum leaves int64 ORs kWindowErrorSum into *error
    kWindowScanMin = 2,     // out: 8 bytes per row, the first best of those rows' values (unspecified while there is none)
    kWindowScanMax = 3
};
constexpr int32_t kWindowErrorBuckets = 1, kWindowErrorSum = 2, kWindowErrorLagOffset = 4, kWindowErrorNthOffset = 8;   // bits of the error word
// bytes of `temp` for n rows: the tile aggregates and their exclusive scan
size_t window_scan_temp_bytes(int32_t n);
// floating: the values are doubles' bits (min in Double.compare order; max: NaN loses to everything, the zeros tie), else int64
void launch_window_scan(WindowScanKind kind, bool floating, const uint64_t* sorted_values, const uint8_t* sorted_nulls, const int32_t* part_flag,
                        int32_t n, void* out, int32_t* error, void* temp, hipStream_t s);

enum WindowFrameEnd { kWindowFrameRow = 0, kWindowFramePeers = 1, kWindowFramePartition = 2 };   // e = i, pe - 1, N - 1

struct WindowFunction {
    int32_t function;          // pa_window_function
    int32_t arg_type;          // ntile: PA_BIGINT / PA_INTEGER; min / max: the argument's type = the output's
    int32_t frame_end;         // aggregates, first_value / last_value / nth_value: WindowFrameEnd
    int32_t offset_type;       // PA_BIGINT / PA_INTEGER
    int32_t width;             // value functions: bytes of one value, 1 / 4 / 8 / 16
    const void* arg_values;    // ntile: the argument channel by held row; value functions: the value channel by held row
    const uint8_t* arg_nulls;  // may be null
    void* out;                 // by sorted index, n x 8 bytes: BIGINT, or DOUBLE for percent_rank / cume_dist; min / max, value functions: n x the type's width
    uint8_t* out_nulls;        // ntile with arg_nulls, sum / min / max with `count`, every lag / lead / nth_value, first_value / last_value with arg_nulls:
                               // n bytes; else null
    const void* scan;          // sum / min / max: the scanned state by sorted index
    const int32_t* count;      // count / sum / min / max: the scanned non-null count; null when the argument has no NULLs
    const void* offset_values;     // lag / lead (null: the offset is 1), nth_value: the offset channel by held row
    const uint8_t* offset_nulls;   // may be null
    const void* default_values;    // lag / lead: the default channel by held row, of the value's type; null: NULL
    const uint8_t* default_nulls;  // may be null
};
// (passed by value as the kernel's argument: 72 + 16 x 104 = 1736 bytes, under the 4 KB a launch takes)
struct WindowFunctionArgs {
    const int32_t* perm;       // sorted index -> held row (read for ntile and the value functions)
    const int32_t* part_flag;
    const int32_t* part_index;
    const int32_t* peer_flag;
    const int32_t* peer_index;
    const int32_t* part_start;
    const int32_t* peer_start;
    int32_t* error;            // a row whose ntile bucket count is <= 0 ORs kWindowErrorBuckets into it; a lag / lead offset < 0
                               // kWindowErrorLagOffset, an nth_value offset < 1 kWindowErrorNthOffset
    int32_t n;
    int32_t count;
    WindowFunction f[kWindowMaxFunctions];
};
static_assert(sizeof(WindowFunction) == 104 && sizeof(WindowFunctionArgs) == 1736, "WindowFunctionArgs: the size the comment states");
void launch_window_functions(const WindowFunctionArgs& a, hipStream_t s);

}  // namespace pa
