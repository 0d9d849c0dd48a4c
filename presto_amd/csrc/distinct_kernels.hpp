// distinct_kernels.hpp -- launchers of distinct_kernels.hip: the growing key table of MarkDistinctOperator / DistinctLimitOperator.
//
// Per page, mark[i] = 1 exactly when no earlier row (of an earlier page, or at a smaller position of this page) has a key that is
// not distinct from row i's (MarkDistinctHash.java:52-69 over GroupByHash.getGroupIds).  The rows marked get the ids
// distinct_count, distinct_count + 1, ... in position order: the reference's group ids.
//
// A key is one canonical 64-bit word per channel (semi_join_kernels.hpp; a VARCHAR's word is its id in the channel's StringInterner)
// plus one bit per channel for NULL, whose word is 0: two rows are not distinct exactly when words and bits are equal.
//
// Table: open addressing, linear probing, one 64-bit word per slot = tag << 32 | ref; tag = the high half of the key's hash,
// ref = id of a key published by an earlier page, or kDistinctPageRef | position in the page being inserted.  ~0 = empty.
#pragma once

#include "common.hpp"
#include "join_kernels.hpp"

namespace pa {

constexpr uint32_t kDistinctPageRef = 0x80000000u;
constexpr int kDistinctRowsPerBlock = 1024;   // rows of one workgroup of the mark / publish passes: 256 lanes x 4 rows

// the canonical form of one page
struct DistinctKeys {
    const uint64_t* words[kMaxJoinChannels];  // per key channel: n words
    const uint8_t* nullbits;                  // per row: bit c = channel c is NULL; null = no NULL in the page
    int32_t ncols;
    int32_t n;
};
// the keys published so far, by id
struct DistinctStore {
    uint64_t* words[kMaxJoinChannels];
    uint8_t* nullbits;
    uint32_t capacity;   // ids the arrays have room for
    uint32_t pad;
};
struct DistinctTable {
    uint64_t* slots;
    uint32_t mask;       // slots - 1 (a power of two)
    uint32_t pad;
};

// Pass 1.  src[c]: the staged key column (VARCHAR: values = the interner's i32 ids, type PA_INTEGER); out[c] = null for a channel
// whose column already is its canonical form (8-byte integers without NULLs: keys.words[c] points at the page).
struct DistinctCanonArgs {
    JoinCol src[kMaxJoinChannels];
    uint64_t* out[kMaxJoinChannels];
    uint8_t* nullbits;   // null when no channel has NULL flags
    int32_t ncols;
    int32_t n;
};
void launch_distinct_canon(const DistinctCanonArgs& a, hipStream_t s);

// Pass 2: every row finds or claims the slot of its key.  Of the rows of this page that share a new key, the slot ends up holding
// the smallest position, whatever order the waves ran in.  slot_of[i] = the slot when row i's position went into it (it may be the
// one that stays), -1 when the row met its key from an earlier page or at a smaller position.
void launch_distinct_insert(const DistinctKeys& keys, const DistinctStore& store, const DistinctTable& table, int32_t* slot_of, hipStream_t s);

// The same pass for an operator that needs the group id of EVERY row (RowNumberOperator): a second instantiation that also writes
// stop_of[i] = the slot row i's probe ended at (n entries).  Once the publish pass has run, that slot holds tag | id.
void launch_distinct_insert_ids(const DistinctKeys& keys, const DistinctStore& store, const DistinctTable& table, int32_t* slot_of, int32_t* stop_of,
                                hipStream_t s);
// ... and behind the publish pass: gids[i] = id of row i's key (GroupByHash.getGroupIds), widened to the 64-bit keys launch_sort_pairs takes
void launch_distinct_group_ids(const DistinctTable& table, const int32_t* stop_of, int32_t n, uint64_t* gids, hipStream_t s);

// Pass 3a: mark[i] (round_up(n, 4) bytes) and the marks of each block of kDistinctRowsPerBlock rows (block_counts)
void launch_distinct_mark(const DistinctTable& table, const int32_t* slot_of, int32_t n, uint8_t* mark, int32_t* block_counts, hipStream_t s);
inline int64_t distinct_blocks(int64_t n) { return (n + kDistinctRowsPerBlock - 1) / kDistinctRowsPerBlock; }

// Pass 3b, after the exclusive scan of block_counts (block_offsets; *page_total = their sum): the row marked with rank r in the page
// gets id = count + r, appends its key to the store at id and rewrites its slot to tag | id; out_positions (may be null: at least
// `limit` entries) [r] = its position for r < limit.  counter_in / counter_out: two device words, {page sequence number << 32 |
// distinct count}: in as the previous page left it, out = {seq, count + *page_total}.  *err = 1 when an id would pass store.capacity
// (nothing is written then).
struct DistinctPublishArgs {
    DistinctKeys keys;
    DistinctStore store;
    DistinctTable table;
    const int32_t* slot_of;
    const uint8_t* mark;
    const int32_t* block_offsets;
    const int32_t* page_total;
    const uint64_t* counter_in;
    uint64_t* counter_out;
    int32_t* out_positions;
    int32_t* err;
    int64_t limit;
    uint32_t seq;
    uint32_t pad;
};
void launch_distinct_publish(const DistinctPublishArgs& a, hipStream_t s);

// Growth: the ids [0, count) of the store into an empty (all ~0) table; stored keys all differ, so nothing is compared
void launch_distinct_rehash(const DistinctStore& store, int32_t ncols, uint32_t count, const DistinctTable& table, hipStream_t s);

}  // namespace pa
