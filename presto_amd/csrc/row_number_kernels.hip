// row_number_kernels.hip -- the passes of RowNumberOperator behind the key table (row_number_kernels.hpp).
#include <hip/hip_runtime.h>

#include "row_number_kernels.hpp"
#include "kernels/pa_device.h"

namespace pa {

// Where the run of equal ids that ends at index `last` (ids[last] == id) begins.  The ids are sorted, so "ids[x] == id" is false and
// then true over x <= last: gallop back in doubling steps until it is false (or the array begins), then bisect.
__device__ __forceinline__ i64 run_head_before(const u64* __restrict__ ids, i64 last, u64 id)
{
    i64 hi = last;    // known: ids[hi] == id
    i64 lo = -1;      // known: ids[lo] != id (or before the array)
    for (i64 step = kRowNumberRowsPerBlock;; step <<= 1) {
        const i64 p = hi - step;
        if (p < 0) break;
        if (ids[p] != id) {
            lo = p;
            break;
        }
        hi = p;
    }
    while (hi - lo > 1) {
        const i64 mid = (lo + hi) >> 1;
        if (ids[mid] == id) hi = mid;
        else lo = mid;
    }
    return hi;
}

// A workgroup takes 1024 consecutive pairs of the sorted order, a lane four consecutive ones.
__global__ __launch_bounds__(256) void k_row_number_rank(RowNumberRankArgs a)
{
    __shared__ i32 wave_last[4];
    __shared__ i32 carry;
    const i32 n = a.n;
    const u64* __restrict__ gids = (const u64*)a.gids;
    const i64 base = (i64)blockIdx.x * kRowNumberRowsPerBlock;
    const i64 j0 = base + (i64)threadIdx.x * 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the head of the run the workgroup's first pair belongs to: its own index unless the run reaches in from the left
    if (threadIdx.x == 0) {
        i64 head = base;
        if (base > 0) {
            const u64 first = gids[base];
            if (gids[base - 1] == first) head = run_head_before(gids, base - 1, first);
        }
        carry = (i32)head;
    }
    u64 k[4];
    i32 head[4];   // the head of pair e's run when it lies among the lane's own pairs, else -1
    i32 mine = -1;
    u64 prev = j0 > 0 && j0 < n ? gids[j0 - 1] : 0ULL;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const i64 j = j0 + e;
        k[e] = j < n ? gids[j] : 0ULL;
        if (j < n && (j == 0 || k[e] != prev)) mine = (i32)j;
        head[e] = mine;
        prev = k[e];
    }
    const u64 next = j0 + 4 < n ? gids[j0 + 4] : 0ULL;
    // inclusive max-scan of the lanes' last heads over the wave, then over the workgroup's waves
    i32 incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const i32 up = __shfl_up(incl, d, 64);
        if (lane >= d) incl = max(incl, up);
    }
    i32 left = __shfl_up(incl, 1, 64);
    if (lane == 0) left = -1;
    if (lane == 63) wave_last[wave] = incl;
    __syncthreads();
    i32 before = carry;   // <= base <= every head found inside the workgroup
    for (int w = 0; w < wave; w++) before = max(before, wave_last[w]);
    left = max(left, before);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const i64 j = j0 + e;
        if (j >= n) break;
        const u64 gid = k[e];
        if (gid >= (u64)a.counts_n) continue;
        const i64 h = head[e] >= 0 ? (i64)head[e] : (i64)left;
        const i64 rn = a.counts[gid] + (j - h) + 1;
        const i32 pos = a.rows[j];
        a.rn[pos] = rn;
        if (a.cap >= 0) a.keep[pos] = rn <= a.cap ? (u8)1 : (u8)0;
        const bool last = j == n - 1 || (e < 3 ? k[e + 1] : next) != gid;
        if (last) a.tails[j] = rn;   // = the group's count before the page + the run's length
    }
}

__global__ __launch_bounds__(256) void k_row_number_update(const u64* __restrict__ gids, const i64* __restrict__ tails, i32 n, i64 cap, i64* __restrict__ counts,
                                                           i64 counts_n)
{
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n; j += (i64)gridDim.x * 256) {
        const u64 gid = gids[j];
        if (j != n - 1 && gids[j + 1] == gid) continue;
        if (gid >= (u64)counts_n) continue;
        const i64 v = tails[j];
        counts[gid] = cap >= 0 && v > cap ? cap : v;
    }
}

__global__ __launch_bounds__(256) void k_row_number_iota(i64 start, i32 n, i64* __restrict__ rn)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) rn[i] = start + i + 1;
}
__global__ __launch_bounds__(256) void k_row_number_positions_iota(i32 n, i32* __restrict__ positions)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) positions[i] = (i32)i;
}

// the keep flags of a lane's four consecutive rows, one bit per row; bytes behind row n - 1 are not looked at
__device__ __forceinline__ u32 keep_bits(const u8* __restrict__ keep, i64 q, i32 n)
{
    const i64 r0 = 4 * q;
    if (r0 >= n) return 0u;
    const u32 w = ((const u32*)keep)[q];
    u32 m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (r0 + j < n && ((w >> (8 * j)) & 0xffu) != 0) m |= 1u << j;
    return m;
}

__global__ __launch_bounds__(256) void k_row_number_keep_counts(const u8* __restrict__ keep, i32 n, i32* __restrict__ block_counts)
{
    __shared__ i32 lds[4];
    i32 c = __popc(keep_bits(keep, (i64)blockIdx.x * 256 + threadIdx.x, n));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(256) void k_row_number_keep_positions(const u8* __restrict__ keep, i32 n, const i32* __restrict__ block_offsets,
                                                                   i32* __restrict__ positions)
{
    __shared__ i32 lds[4];
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    const u32 m = keep_bits(keep, q, n);
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
    i64 at = (i64)block_offsets[blockIdx.x] + before + incl - cnt;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if ((m >> j) & 1u) positions[at++] = (i32)(4 * q + j);
}

static inline int row_number_grid(int64_t work)
{
    int64_t g = (work + 255) / 256;
    if (g < 1) g = 1;
    if (g > 256 * 16) g = 256 * 16;
    return (int)g;
}

void launch_row_number_rank(const RowNumberRankArgs& a, hipStream_t s)
{
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_row_number_rank, (int)row_number_blocks(a.n), 256, 0, s, a);
    PA_HIP(hipGetLastError());
}
void launch_row_number_update(const uint64_t* gids, const int64_t* tails, int32_t n, int64_t cap, int64_t* counts, int64_t counts_n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_row_number_update, row_number_grid(n), 256, 0, s, (const u64*)gids, (const i64*)tails, n, (i64)cap, (i64*)counts, (i64)counts_n);
    PA_HIP(hipGetLastError());
}
void launch_row_number_iota(int64_t start, int32_t n, int64_t* rn, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_row_number_iota, row_number_grid(n), 256, 0, s, (i64)start, n, (i64*)rn);
    PA_HIP(hipGetLastError());
}
void launch_row_number_positions_iota(int32_t n, int32_t* positions, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_row_number_positions_iota, row_number_grid(n), 256, 0, s, n, positions);
    PA_HIP(hipGetLastError());
}
void launch_row_number_keep_counts(const uint8_t* keep, int32_t n, int32_t* block_counts, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_row_number_keep_counts, (int)row_number_blocks(n), 256, 0, s, keep, n, block_counts);
    PA_HIP(hipGetLastError());
}
void launch_row_number_keep_positions(const uint8_t* keep, int32_t n, const int32_t* block_offsets, int32_t* positions, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_row_number_keep_positions, (int)row_number_blocks(n), 256, 0, s, keep, n, block_offsets, positions);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
