// distinct_kernels.hip -- the growing key table behind MarkDistinctOperator, DistinctLimitOperator and RowNumberOperator (distinct_kernels.hpp).
//
// Why no claim / publish protocol is needed inside the insert pass, although workgroups on different XCDs race on the slots:
//   * a slot word is read and written with agent-scope atomics only (load, compare-and-swap, min);
//   * what a slot REFERS to is never written during the pass: a page ref points into the page's canonical key columns (written by
//     the launch before), an id into the key store (written by the publish passes of earlier pages);
//   * a slot changes in two ways only: empty -> {tag, page ref} by the CAS of one row, and {tag, page ref p} -> {tag, page ref p'}
//     with p' < p by the min of a row whose key equals row p's.  So a claimed slot keeps its key for the rest of the pass, every
//     row of that key stops at it, and after the pass it holds the smallest of their positions -- whatever order the waves ran in.
// The mark and publish passes are launches of their own: they see the finished table.
#include <hip/hip_runtime.h>

#include "distinct_kernels.hpp"
#include "kernels/pa_device.h"
#include "kernels/pa_canon.h"

namespace pa {

#define DISTINCT_EMPTY (~0ULL)

__device__ __forceinline__ u64 slot_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void slot_store(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// true: the slot was `expected` and is `desired` now; false: `expected` = what it holds instead
__device__ __forceinline__ bool slot_cas(u64* p, u64& expected, u64 desired)
{
    return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the key's hash: low bits = home slot, high half = tag.  Internal: it need not agree with $hashvalue.
template <class Words>
__device__ __forceinline__ u64 distinct_hash(const Words& words, int ncols, i64 i, u32 nullbits)
{
    u64 h = (u64)nullbits * PA_P3;
    for (int c = 0; c < ncols; c++) h = pa_rotl64(h, 27) * PA_P1 + pa_murmur3_fmix(words[c][i] + PA_P5);
    return pa_murmur3_fmix(h);
}

__global__ __launch_bounds__(256) void k_distinct_canon(DistinctCanonArgs a)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (i64)gridDim.x * 256) {
        u32 bits = 0;
        for (int c = 0; c < a.ncols; c++) {
            const JoinCol& k = a.src[c];
            const bool null = k.nulls != nullptr && k.nulls[i] != 0;
            if (null) bits |= 1u << c;
            if (a.out[c] != nullptr) a.out[c][i] = null ? 0ULL : semi_canon_bits(k.type, k.values, i);
        }
        if (a.nullbits != nullptr) a.nullbits[i] = (u8)bits;
    }
}

__device__ __forceinline__ bool distinct_eq_page(const DistinctKeys& k, i64 i, u32 nb, i64 p)
{
    if (k.nullbits != nullptr && k.nullbits[p] != nb) return false;
    for (int c = 0; c < k.ncols; c++)
        if (k.words[c][i] != k.words[c][p]) return false;
    return true;
}
__device__ __forceinline__ bool distinct_eq_store(const DistinctKeys& k, i64 i, u32 nb, const DistinctStore& st, u32 id)
{
    if (st.nullbits[id] != nb) return false;
    for (int c = 0; c < k.ncols; c++)
        if (k.words[c][i] != st.words[c][id]) return false;
    return true;
}

// A workgroup takes 1024 consecutive rows, a lane four of them 256 apart (coalesced key loads).  The four home slots are loaded
// before the first is looked at: the pass is bound by the latency of dependent slot loads.
// kStops (RowNumberOperator): stop_of[i] = the slot row i's probe ended at, whether the row may be first of its key or not -- the slot
// that holds the key's id once the publish pass has run.  Without it the body is what MarkDistinct / DistinctLimit have always launched.
template <bool kStops>
__device__ __forceinline__ void distinct_insert_rows(const DistinctKeys& keys, const DistinctStore& store, const DistinctTable& t, i32* __restrict__ slot_of,
                                                     i32* __restrict__ stop_of)
{
    const i64 base = (i64)blockIdx.x * kDistinctRowsPerBlock + threadIdx.x;
    u64 h[4], v[4];
    u32 nb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const i64 i = base + j * 256;
        if (i >= keys.n) continue;
        nb[j] = keys.nullbits != nullptr ? keys.nullbits[i] : 0u;
        h[j] = distinct_hash(keys.words, keys.ncols, i, nb[j]);
        v[j] = slot_load((u64*)t.slots + ((u32)h[j] & t.mask));
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const i64 i = base + j * 256;
        if (i >= keys.n) continue;
        const u64 tag = h[j] & 0xffffffff00000000ULL;
        const u64 mine = tag | (u64)(kDistinctPageRef | (u32)i);
        u32 pos = (u32)h[j] & t.mask;
        u64 cur = v[j];
        bool candidate = false;   // this row's position went into the slot: it may be the one that stays
        for (;;) {
            if (cur == DISTINCT_EMPTY) {
                candidate = slot_cas((u64*)t.slots + pos, cur, mine);
                if (candidate) break;
                continue;   // somebody else's key or row got there first: look at what the slot holds now
            }
            if ((cur & 0xffffffff00000000ULL) == tag) {
                const u32 ref = (u32)cur;
                if ((ref & kDistinctPageRef) != 0) {
                    const u32 p = ref & ~kDistinctPageRef;
                    if (distinct_eq_page(keys, i, nb[j], (i64)p)) {
                        // the smallest position wins.  `cur` was just read: a holder already below this row stays (in a page of one
                        // key nearly every row leaves here without an atomic)
                        candidate = p > (u32)i;
                        if (candidate) __hip_atomic_fetch_min((u64*)t.slots + pos, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                }
                else if (distinct_eq_store(keys, i, nb[j], store, ref)) break;
            }
            pos = (pos + 1) & t.mask;
            cur = slot_load((u64*)t.slots + pos);
        }
        // a row that met its key from an earlier page, or at a smaller position of this one, is out: the mark pass need not look
        slot_of[i] = candidate ? (i32)pos : -1;
        if (kStops) stop_of[i] = (i32)pos;
    }
}

__global__ __launch_bounds__(256) void k_distinct_insert(DistinctKeys keys, DistinctStore store, DistinctTable t, i32* __restrict__ slot_of)
{
    distinct_insert_rows<false>(keys, store, t, slot_of, nullptr);
}
__global__ __launch_bounds__(256) void k_distinct_insert_ids(DistinctKeys keys, DistinctStore store, DistinctTable t, i32* __restrict__ slot_of,
                                                             i32* __restrict__ stop_of)
{
    distinct_insert_rows<true>(keys, store, t, slot_of, stop_of);
}

__device__ __forceinline__ i32 block_sum_256(i32 mine, i32* lds)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mine;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// A lane marks four consecutive rows with one 4-byte store (as semi_join_kernels.hip); slot_of is padded to a multiple of 4.
__global__ __launch_bounds__(256) void k_distinct_mark(DistinctTable t, const i32* __restrict__ slot_of, i32 n, u8* __restrict__ mark,
                                                       i32* __restrict__ block_counts)
{
    __shared__ i32 lds[4];
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 r0 = 4 * q;
    u32 m = 0;
    if (r0 < n) {
        const pa_i32x4 s = ((const pa_i32x4*)slot_of)[q];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (r0 + j >= n || s[j] < 0) continue;
            const u64 cur = slot_load((u64*)t.slots + (u32)s[j]);
            if ((u32)cur == (kDistinctPageRef | (u32)(r0 + j))) m |= 1u << (8 * j);
        }
        ((u32*)mark)[q] = m;
    }
    const i32 total = block_sum_256(__popc(m), lds);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_distinct_publish(DistinctPublishArgs a)
{
    __shared__ i32 lds[4];
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 r0 = 4 * q;
    const i32 n = a.keys.n;
    const u32 m = r0 < n ? ((const u32*)a.mark)[q] : 0u;
    // exclusive prefix of the marks over the workgroup's rows, in position order
    const i32 cnt = __popc(m);
    i32 incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const i32 up = __shfl_up(incl, d, 64);
        if ((i32)(threadIdx.x & 63) >= d) incl += up;
    }
    if ((threadIdx.x & 63) == 63) lds[threadIdx.x >> 6] = incl;
    __syncthreads();
    i32 before = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) before += lds[w];
    i64 rank = (i64)a.block_offsets[blockIdx.x] + before + incl - cnt;
    const u32 count = (u32)*a.counter_in;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.counter_out = ((u64)a.seq << 32) | (u64)(count + (u32)*a.page_total);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (((m >> (8 * j)) & 1u) == 0) continue;
        const i64 i = r0 + j;
        const u64 id = (u64)count + (u64)rank;
        if (id >= (u64)a.store.capacity) {
            *a.err = 1;
            return;
        }
        for (int c = 0; c < a.keys.ncols; c++) a.store.words[c][id] = a.keys.words[c][i];
        a.store.nullbits[id] = a.keys.nullbits != nullptr ? a.keys.nullbits[i] : (u8)0;
        u64* slot = (u64*)a.table.slots + (u32)a.slot_of[i];
        slot_store(slot, (slot_load(slot) & 0xffffffff00000000ULL) | id);
        if (a.out_positions != nullptr && rank < a.limit) a.out_positions[rank] = (i32)i;
        rank++;
    }
}

// After the publish pass every slot a probe ended at holds tag | id: the group id of every row, as a 64-bit sort key
__global__ __launch_bounds__(256) void k_distinct_group_ids(DistinctTable t, const i32* __restrict__ stop_of, i32 n, u64* __restrict__ gids)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) gids[i] = (u64)(u32)slot_load((u64*)t.slots + (u32)stop_of[i]);
}

__global__ __launch_bounds__(256) void k_distinct_rehash(DistinctStore store, i32 ncols, u32 count, DistinctTable t)
{
    for (i64 id = (i64)blockIdx.x * 256 + threadIdx.x; id < (i64)count; id += (i64)gridDim.x * 256) {
        const u64 h = distinct_hash(store.words, ncols, id, store.nullbits[id]);
        const u64 mine = (h & 0xffffffff00000000ULL) | (u64)id;
        u32 pos = (u32)h & t.mask;
        for (;;) {
            u64 cur = slot_load((u64*)t.slots + pos);
            if (cur == DISTINCT_EMPTY && slot_cas((u64*)t.slots + pos, cur, mine)) break;
            pos = (pos + 1) & t.mask;
        }
    }
}

static inline int distinct_grid(int64_t work)
{
    int64_t g = (work + 255) / 256;
    if (g < 1) g = 1;
    if (g > 256 * 16) g = 256 * 16;
    return (int)g;
}

void launch_distinct_canon(const DistinctCanonArgs& a, hipStream_t s)
{
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_distinct_canon, distinct_grid(a.n), 256, 0, s, a);
    PA_HIP(hipGetLastError());
}
void launch_distinct_insert(const DistinctKeys& keys, const DistinctStore& store, const DistinctTable& table, int32_t* slot_of, hipStream_t s)
{
    if (keys.n <= 0) return;
    hipLaunchKernelGGL(k_distinct_insert, (int)distinct_blocks(keys.n), 256, 0, s, keys, store, table, slot_of);
    PA_HIP(hipGetLastError());
}
void launch_distinct_insert_ids(const DistinctKeys& keys, const DistinctStore& store, const DistinctTable& table, int32_t* slot_of, int32_t* stop_of, hipStream_t s)
{
    if (keys.n <= 0) return;
    hipLaunchKernelGGL(k_distinct_insert_ids, (int)distinct_blocks(keys.n), 256, 0, s, keys, store, table, slot_of, stop_of);
    PA_HIP(hipGetLastError());
}
void launch_distinct_group_ids(const DistinctTable& table, const int32_t* stop_of, int32_t n, uint64_t* gids, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_distinct_group_ids, distinct_grid(n), 256, 0, s, table, stop_of, n, (u64*)gids);
    PA_HIP(hipGetLastError());
}
void launch_distinct_mark(const DistinctTable& table, const int32_t* slot_of, int32_t n, uint8_t* mark, int32_t* block_counts, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_distinct_mark, (int)distinct_blocks(n), 256, 0, s, table, slot_of, n, mark, block_counts);
    PA_HIP(hipGetLastError());
}
void launch_distinct_publish(const DistinctPublishArgs& a, hipStream_t s)
{
    if (a.keys.n <= 0) return;
    hipLaunchKernelGGL(k_distinct_publish, (int)distinct_blocks(a.keys.n), 256, 0, s, a);
    PA_HIP(hipGetLastError());
}
void launch_distinct_rehash(const DistinctStore& store, int32_t ncols, uint32_t count, const DistinctTable& table, hipStream_t s)
{
    if (count == 0) return;
    hipLaunchKernelGGL(k_distinct_rehash, distinct_grid(count), 256, 0, s, store, ncols, count, table);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
