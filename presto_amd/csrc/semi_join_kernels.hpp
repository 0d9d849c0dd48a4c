// semi_join_kernels.hpp -- launchers of semi_join_kernels.hip: the set's canonical keys and the probe's mark pass.
#pragma once

#include "common.hpp"
#include "join_kernels.hpp"

namespace pa {

// Canonical 64-bit form of a set value under IS NOT DISTINCT FROM (ChannelSet.contains -> positionNotDistinctFromRow): integer types
// and short DECIMAL as the value, BOOLEAN as 0 / 1, DOUBLE / REAL as their bits with every NaN one bit pattern and -0.0 as +0.0.
// Two values are not distinct exactly when their canonical keys are equal, so the set of a non-VARCHAR channel is a lookup source
// over one BIGINT key -- the keyed layouts of the join build (bitmap, rank index, key slots) as they are.
// out[i] = canonical key of row i; *any_null (device, zeroed by the caller) = 1 when some row is NULL.
void launch_semi_canon(const JoinCol& key, int32_t n, uint64_t* out, int32_t* any_null, hipStream_t s);
// *any_null = 1 when nulls[0 .. n) holds a non-zero byte (VARCHAR sets)
void launch_semi_any_null(const uint8_t* nulls, int32_t n, int32_t* any_null, hipStream_t s);

// Which structure of the lookup source answers "is k in the set"
enum SemiLayout {
    SEMI_EMPTY = 0,   // no build position: every mark is false (HashSemiJoinOperator.java:190-196)
    SEMI_BITMAP = 1,  // canonical integer key in the existence bitmap (JoinKeyBitmap)
    SEMI_SLOTS = 2,   // canonical key in the keyed slot table (JoinKeySlot): presence only, first match ends the probe
    SEMI_TAGGED = 3,  // VARCHAR: the tagged table of the generic join build, byte equality against the build column
};
struct SemiProbeArgs {
    JoinCol key;                 // probe key column, flat / varwidth on the device
    int32_t n;
    int32_t layout;              // SemiLayout
    int32_t miss_is_null;        // ChannelSet.containsNull(): a key not found marks NULL
    int32_t null_is_null;        // the set is not empty: a NULL key marks NULL
    uint8_t* mark;               // round_up(n, 4) bytes: 1 = true
    uint8_t* mark_null;          // round_up(n, 4) bytes, or null when no mark can be NULL
    int32_t* any_null_mark;      // device word set to 1 when some mark is NULL (with mark_null)
    JoinKeyBitmap bitmap;        // SEMI_BITMAP
    const JoinKeySlot* slots;    // SEMI_SLOTS
    uint32_t mask, wrap;
    JoinCol build_key;           // SEMI_TAGGED
    const uint64_t* tagged;
    const int64_t* probe_hash;   // SEMI_TAGGED: the raw hash of every probe row (launch_hash_page)
};
// one pass over the probe key column; returns the name of the kernel launched (pa_op_kernel_name)
const char* launch_semi_mark(const SemiProbeArgs& a, hipStream_t s);

// Distinct non-NULL values of a built set: popcount of the bitmap, occupied slots of the key slot table or of the tagged table
// (each holds one entry per distinct key).  out: device u64, zeroed by the caller.
void launch_semi_count_bits(const uint64_t* words, int64_t nwords, unsigned long long* out, hipStream_t s);
void launch_semi_count_slots(const JoinKeySlot* slots, int64_t size, unsigned long long* out, hipStream_t s);
void launch_semi_count_tagged(const uint64_t* tagged, int64_t size, unsigned long long* out, hipStream_t s);

}  // namespace pa
