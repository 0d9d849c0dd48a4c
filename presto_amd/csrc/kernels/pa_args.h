// pa_args.h -- the argument blocks of the generated kernels, defined ONCE: every generated kernel takes one block by value, the host
// fills the same struct it launches with (void* params[] = {&a}).  Plain C++: the host code includes this file as it is, the statically
// compiled kernels get it through pa_device.h, and the hiprtc translation units (which have no include path) carry its text in front
// of pa_device.h's (csrc/Makefile, pa_device_embed.inc).
#pragma once

// Device code spells the 64-bit types `long long` (what the HIP builtins take).  The operators' buffers are <cstdint>'s int64_t /
// uint64_t, which on LP64 is `long`: a host file that fills the blocks defines PA_ARGS_STDINT in front of its #include, so that its
// pointers convert.  Same size and alignment either way -- one layout -- and one spelling per translation unit (#pragma once).
#ifdef PA_ARGS_STDINT
#include <cstdint>
typedef int64_t i64;
typedef uint64_t u64;
#else
typedef long long i64;
typedef unsigned long long u64;
#endif
typedef int i32;
typedef unsigned int u32;
typedef unsigned char u8;
typedef u32 pa_u32x4 __attribute__((ext_vector_type(4)));

#define PA_MAX_CHANNELS 32
#define PA_MAX_BUILD_CHANNELS 8
// channels of the build page and the probe page of a nested-loop join together
#define PA_NL_MAX_CHANNELS 64

// Kernel argument block of the fused scan-filter-project-aggregate kernels.
struct PaFusedArgs {
    const void* v[PA_MAX_CHANNELS];   // column values (FLAT) / bytes (VARWIDTH)
    const i32* o[PA_MAX_CHANNELS];    // VARWIDTH offsets
    const u8* nl[PA_MAX_CHANNELS];    // nulls (1 B / row) or nullptr
    i64 n;                            // rows in this page
    i32 vec;                          // 1: every used buffer is 16-B aligned -> 4 rows / lane / step
    i32 pad;
    u64* slab;                        // per-workgroup partial states of this launch
    u64* gt_tag;                      // global group table: 0 empty | hash<<2|1 busy | hash<<2|3 ready
    u64* gt_keys;                     // [capacity][W]
    u64* gt_words;                    // [NW][capacity] accumulator words
    u32 gt_mask;                      // capacity - 1
    i32 gt_max_fill;
    i32* gt_count;                    // groups in the table
    i32* err;                         // first device-raised pa_status
    u64* overflow_rows;               // rows that missed the LDS table (drives mode escalation)
    const i32* row_list;              // GT variant: process these rows (of this launch's range) instead of all n
    i64 n_list;
    i32* spill_rows;                  // GT variant: rows whose group did not fit the table (redone after a rehash)
    u32* spill_count;
    // Replicas of the group table: workgroup b works on replica b & gt_rep_mask (each a full table of gt_mask + 1 slots,
    // laid out one after the other in gt_tag / gt_keys / gt_words).  Atomics of many rows on few addresses retire at
    // ~0.15 M/s per address on this part; R replicas divide the pressure per address by R.  The host folds the
    // replicas into one table before the result is read.
    u32 gt_rep_mask;
    u32 part_mask;                    // hash-partitioning pass: partitions - 1 (partition id part_mask + 1 = row filtered out)
    i32* gt_rep_count;                // groups of replica r >= 1 at [r]; replica 0 counts in gt_count
    i32* part_ids;                    // hash-partitioning pass: partition of every row of the launch
    i32 list_blocked;                 // row_list is cut into one contiguous slice per workgroup (partition-ordered lists)
    i32 pad3;
    // Partition-owned tables (LDSP variant): workgroup p aggregates the rows [part_first[p], part_first[p + 1]) of the
    // partition-ordered columns into an LDS table it LOADS from and STORES to sub_*[p] -- the groups of partition p live nowhere
    // else, so neither the row loop nor the hand-over to HBM needs an atomic on HBM.  Layout per partition: PA_LC tags,
    // PA_LC x PA_KW key words, PA_LC x PA_NW accumulator words (slot-major), one group count.
    u64* sub_tag;
    u64* sub_keys;
    u64* sub_words;
    i32* sub_count;
    const i64* part_first;
    // Probe stage (fused FilterAndProject -> LookupJoin -> aggregation over a lookup source with ONE integer key and no
    // duplicate keys): the keyed probe-side table of join_kernels.hpp (16 B slots: key, head, next), the build side's key
    // existence bitmap (null = none) and the build columns the aggregation reads, indexed by build position.
    const void* jslots;
    const u64* jbits;
    i64 jmin;
    u64 jrange;
    u32 jmask;
    i32 jrows;                        // build positions (the build-row table of the BROW variant has this many slots)
    u32 jwrap;                        // probe sequences wrap inside (pos & ~jwrap): jmask, or the partition size - 1 of a partitioned build
    u32 jpad;
    const void* bv[PA_MAX_BUILD_CHANNELS];
    const u8* bn[PA_MAX_BUILD_CHANNELS];
    // key rank index (join_kernels.hpp JoinRankIndex; null = none, the slot table answers): 16-byte words {64 key bits, build keys
    // below the word} over [jmin, jmin + jrange], and rank -> build position (null: the rank is the position)
    const pa_u32x4* jrank;
    const i32* jrank_rows;
    // pa_fused_ranges: a table of row ranges taken in place (entry layout: op_fused.cpp range_entry_words)
    const u64* ranges;
    i64 n_ranges;
};

// Kernel argument block of the generated FilterAndProject kernels (op_filter_project.cpp).
struct PaFpArgs {
    const void* v[PA_MAX_CHANNELS];
    const i32* o[PA_MAX_CHANNELS];
    const u8* nl[PA_MAX_CHANNELS];
    void* out_v[PA_MAX_CHANNELS];   // per projection: output values (worst case n entries)
    u8* out_nl[PA_MAX_CHANNELS];    // per projection: output nulls or nullptr
    i64 n;
    i32 vec;
    i32 pad;
    u8* sel4;                       // 4 selection bits per row quad (filter result, PageFilter.filter)
    i32* tile_counts;               // selected rows per 1024-row tile
    const i32* tile_offsets;        // exclusive scan of tile_counts
    i32* positions;                 // SelectedPositions.positions (ascending), worst case n entries
    i32* err;
    const u64* dyn_bits;            // dynamic filter from a join's build side: existence bitmap over [dyn_min, dyn_min + dyn_range]
    i64 dyn_min;
    u64 dyn_range;
    // probe stage (FilterAndProject -> LookupJoin in one pass, op_filter_project.cpp): the keyed probe-side table, its key bitmap,
    // and the build columns the output carries, as in PaFusedArgs
    const void* jslots;
    const u64* jbits;
    i64 jmin;
    u64 jrange;
    u32 jmask;
    u32 jwrap;
    const void* bv[PA_MAX_BUILD_CHANNELS];
    const u8* bn[PA_MAX_BUILD_CHANNELS];
    const pa_u32x4* jrank;          // key rank index, as in PaFusedArgs
    const i32* jrank_rows;
};

// Kernel argument block of the generated nested-loop pair kernels (op_nested_loop.cpp): the pairs of the probe rows [i0, i0 + n) with the
// build rows [j0, j0 + m).  Channels [0, nb) are the build page's, [nb, nb + np) the probe page's.
struct PaNlArgs {
    const void* v[PA_NL_MAX_CHANNELS];
    const i32* o[PA_NL_MAX_CHANNELS];
    const u8* nl[PA_NL_MAX_CHANNELS];
    i32 i0, n, j0, m;
    i32* counts;                    // count form: pairs the filter keeps, per probe row of the rectangle
    const i32* offsets;             // emit form: exclusive scan of counts
    i32* probe_idx;                 // emit form: the kept pairs, probe-major
    i32* build_pos;
    i32* err;
};

// Blocks are passed by value as kernel arguments: bytes, copied as they are.  (The layout itself has no second copy to be compared with.)
static_assert(__is_trivially_copyable(PaFusedArgs) && __is_trivially_copyable(PaFpArgs) && __is_trivially_copyable(PaNlArgs),
              "kernel argument blocks are copied bytewise");
