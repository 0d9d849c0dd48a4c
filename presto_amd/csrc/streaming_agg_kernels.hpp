// streaming_agg_kernels.hpp -- launchers of streaming_agg_kernels.hip: the passes of StreamingAggregationOperator (op_streaming_agg.cpp).
//
// The input arrives grouped: a RUN is a maximal sequence of consecutive rows that are pairwise NOT DISTINCT on the group channels, and
// the operator's result is one row per run.  No table: per page of n rows, in page order,
//   flags     flag[i] = 1 when row i IS DISTINCT FROM row i - 1 on some group channel -- ONE launch over all channels; row 0 is compared
//             with the first-row key of the run the last page left open (the carry), and is never flagged when there is none.
//   scan      idx = the exclusive scan of the flags (scan_kernels.hpp), so that the run of row i is idx[i] + flag[i].  With an open run
//             carried in, run 0 is that run (it has no row of this page when flag[0] is set); without, run 0 starts at row 0.  The
//             scan's total -- the flags of the page -- is the number of runs that CLOSE in this page: every run but the last.
//   starts    start[r] = the first row of run r (start[0] = 0 also where run 0 is the carried one: a placeholder the operator patches).
//   reduce    the segmented reduction of every aggregate, built as window_kernels.hip builds its scans: the state of every tile of
//             kStreamAggTile rows -> one workgroup scans the tile states, seeded with the carried state -> apply.  All aggregates go
//             through one launch of each pass (blockIdx.y = the aggregate).  The apply pass recomputes the tile's prefix states in
//             registers and STORES ONLY AT RUN ENDS: the finished value of run r into the aggregate's output column at r, and the state
//             at row n - 1 into the carry for the next page.  No per-row state array exists.
// Every array element has one writer per launch and no launch reads what it writes (the carry is double-buffered); nothing is carried
// between workgroups of a launch and nothing spins.  The only atomic is the OR into the error word.  The number of launches per page does
// not depend on the number of runs.
//
// State (16 bytes, as the window scans'): {u64 a, i32 b, i32 f}; bit 0 of f = "a run starts inside what this state covers".
//   count            a = the counted rows
//   sum over integers (b, a) = the 96-bit sum, a its low word: exact, so "does this prefix fit int64" is asked of every row;
//                    bit 1 of f = some row counted
//   sum over DOUBLE / REAL, every avg    a = the bits of the double running sum, (f >> 1, b) = the 63-bit count of counted rows
//   min / max        a = the held value's bits (at the type's width, zero-extended), bit 1 of f = there is one
// Algorithmic bytes per row: flags 2 x the key (row i and i - 1; the second read hits the cache) + 4 written; scan 4 + 4; starts 8;
// per aggregate the argument (+ NULL byte, + mask bytes) twice and the flags twice (4 + 4); stores per RUN, not per row.
#pragma once

#include "common.hpp"

namespace pa {

constexpr int kStreamAggTile = 1024;        // rows of one workgroup of the reduction: 256 lanes x 4 consecutive rows
constexpr int kStreamAggMaxKeys = 8;
constexpr int kStreamAggMaxAggregates = 16;

struct StreamAggState {
    uint64_t a;
    int32_t b;
    int32_t f;
};
static_assert(sizeof(StreamAggState) == 16, "StreamAggState: the 16-byte state");

// bits of the error word
constexpr int32_t kStreamAggErrorClosed = 1;   // a run that closes in this page (or is finished) has no result: a prefix of its sum left int64,
                                               // or its INTEGER sum does not fit the INTEGER column
constexpr int32_t kStreamAggErrorOpen = 2;     // a prefix of the sum of the run this page leaves open left int64

struct StreamAggKey {
    int32_t type;
    int32_t pad;
    const void* values;         // the page's column
    const int32_t* offsets;
    const uint8_t* nulls;       // may be null
    const void* carry_values;   // a one-row column: the first row of the open run (read only when `open`)
    const int32_t* carry_offsets;
    const uint8_t* carry_nulls; // may be null
};
struct StreamAggFlagArgs {
    StreamAggKey k[kStreamAggMaxKeys];
    int32_t count;
    int32_t n;
    int32_t open;               // a run is carried in
    int32_t pad;
    int32_t* flags;             // out, n entries
};
// Rows compare as kernels/pa_row_distinct.h states it for IS DISTINCT FROM: both NULL = equal; DOUBLE / REAL: any NaN equals any NaN,
// -0.0 equals +0.0; VARCHAR: length and bytes; BOOLEAN: zero / non-zero; a short DECIMAL as its 8-byte value.
void launch_stream_agg_flags(const StreamAggFlagArgs& a, hipStream_t s);

// start[idx[i] + flag[i]] = i for every flagged i; start[0] = 0.  start: n + 1 entries.
void launch_stream_agg_starts(const int32_t* flags, const int32_t* idx, int32_t n, int32_t* start, hipStream_t s);

enum StreamAggKind { kStreamAggCount = 0, kStreamAggSumInt = 1, kStreamAggSumDouble = 2, kStreamAggMin = 3, kStreamAggMax = 4 };
// min / max keep the first value and take a later one that compares strictly smaller / larger under the type's comparison operator:
// integers as int64; DOUBLE / REAL in Double.compare order -- -0.0 below +0.0, every NaN one value above +infinity -- for min AND max
// (tests/agg_model.py; NOT launch_window_scan's max, under which a NaN loses to everything)
enum StreamAggCompare { kStreamAggCmpInt = 0, kStreamAggCmpDouble = 1, kStreamAggCmpFloat = 2 };

struct StreamAggFn {
    int32_t kind;               // StreamAggKind
    int32_t fn;                 // pa_agg_fn (count(*) ignores the argument's NULLs; sum and avg differ in what they store)
    int32_t in_type;            // pa_type of the argument
    int32_t cmp;                // StreamAggCompare (min / max)
    const void* values;         // the argument channel; null for count(*)
    const uint8_t* nulls;       // may be null
    const uint8_t* mask_values; // the BOOLEAN mask channel or null; a NULL mask is false
    const uint8_t* mask_nulls;  // may be null
    void* out;                  // by run: the result column at its type's width (count: BIGINT; sum: the argument's type; avg: DOUBLE, REAL for REAL;
                                // min / max: the argument's type)
    uint8_t* out_nulls;         // by run; null for the counts
};
// (passed by value as the kernels' argument: 80 + 16 x 64 = 1104 bytes, under the 4 KB a launch takes)
struct StreamAggArgs {
    const int32_t* flags;
    const int32_t* idx;
    const int32_t* closed;            // device: the scan's total = the runs that close in this page
    const StreamAggState* carry_in;   // per aggregate: the state of the open run (read only when `open`)
    StreamAggState* carry_out;        // per aggregate: the state at row n - 1
    StreamAggState* tile_acc;         // [aggregate][tile]
    StreamAggState* tile_front;       // [aggregate][tile]
    int32_t* error;
    int32_t n;
    int32_t tiles;
    int32_t count;
    int32_t open;
    StreamAggFn f[kStreamAggMaxAggregates];
};
static_assert(sizeof(StreamAggFn) == 64 && sizeof(StreamAggArgs) == 1104, "StreamAggArgs: the size the comment states");
inline int32_t stream_agg_tiles(int32_t n) { return (int32_t)(((int64_t)n + kStreamAggTile - 1) / kStreamAggTile); }
// the three launches of the reduction; a.tile_acc / a.tile_front: count x tiles states each
void launch_stream_agg_reduce(const StreamAggArgs& a, hipStream_t s);
// finish: the open run's row -- out[0] / out_nulls[0] of every aggregate from a.carry_in; reads nothing else of `a` but error, count, f
void launch_stream_agg_finish(const StreamAggArgs& a, hipStream_t s);

}  // namespace pa
