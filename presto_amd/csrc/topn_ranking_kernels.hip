// topn_ranking_kernels.hip -- the passes of TopNRankingOperator (topn_ranking_kernels.hpp).
#include <hip/hip_runtime.h>

#include "topn_ranking_kernels.hpp"
#include "kernels/pa_row_distinct.h"

namespace pa {

namespace {

// The arrival filter.  A lane takes four consecutive rows: two 16-byte loads of ids, two of images, four independent gathers of
// bound[] in flight, one 4-byte store of keep flags.  Algorithmic bytes per row: 8 (id) + 8 (image) + 1 (flag) + the gather of
// bound[gid], which hits L2 while the partitions' bounds (8 B each) fit there.  No LDS, no atomics, no dependence between lanes.
__global__ __launch_bounds__(256) void k_topn_ranking_filter(const u64* __restrict__ gids, const u64* __restrict__ images, const u64* __restrict__ bound,
                                                             i64 bound_n, i32 n, u8* __restrict__ keep)
{
    const i64 q = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 r0 = 4 * q;
    if (r0 >= n) return;
    u64 g[4], k[4];
    if (r0 + 4 <= n) {
        const ulonglong2 g01 = ((const ulonglong2*)gids)[2 * q], g23 = ((const ulonglong2*)gids)[2 * q + 1];
        const ulonglong2 k01 = ((const ulonglong2*)images)[2 * q], k23 = ((const ulonglong2*)images)[2 * q + 1];
        g[0] = g01.x; g[1] = g01.y; g[2] = g23.x; g[3] = g23.y;
        k[0] = k01.x; k[1] = k01.y; k[2] = k23.x; k[3] = k23.y;
    }
    else {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool in = r0 + e < n;
            g[e] = in ? gids[r0 + e] : ~0ULL;
            k[e] = in ? images[r0 + e] : 0ULL;
        }
    }
    u64 b[4];
#pragma unroll
    for (int e = 0; e < 4; e++) b[e] = g[e] < (u64)bound_n ? bound[g[e]] : ~0ULL;
    u32 w = 0;
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (k[e] <= b[e]) w |= 1u << (8 * e);
    ((u32*)keep)[q] = w;   // (flags behind row n - 1 are never looked at)
}

// differs from the sorted row before under the comparator's identity: one NaN, two zeros
__global__ __launch_bounds__(256) void k_topn_ranking_differs(i32 type, const void* __restrict__ values, const i32* __restrict__ offsets,
                                                              const u8* __restrict__ nulls, const i32* __restrict__ perm, i32 n, u8* __restrict__ differs)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x + 1; i < n; i += (i64)gridDim.x * 256)
        if (row_distinct<false>(type, values, offsets, nulls, perm[i - 1], perm[i])) differs[i] = 1;
}

__global__ __launch_bounds__(256) void k_topn_ranking_heads(const u64* __restrict__ gids, const u8* __restrict__ differs, i32 n, i32* __restrict__ run_start,
                                                            i64 run_start_n, i32* __restrict__ peer_flag)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const u64 g = gids[i];
        const bool head = i == 0 || gids[i - 1] != g;
        if (head && g < (u64)run_start_n) run_start[g] = (i32)i;
        if (peer_flag) peer_flag[i] = head || differs[i] ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_topn_ranking_peer_starts(const i32* __restrict__ peer_flag, const i32* __restrict__ peer_index, i32 n,
                                                                  i32* __restrict__ peer_start)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
        if (peer_flag[i]) peer_start[peer_index[i]] = (i32)i;
}

__global__ __launch_bounds__(256) void k_topn_ranking_rank(TopNRankingRankArgs a)
{
    const i32 n = a.n;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const u64 g = a.sorted_gids[i];
        if (g >= (u64)a.run_start_n) {   // (cannot happen unless the table failed: such a row is kept unnumbered rather than read out of bounds)
            a.ranking[i] = 0;
            a.keep[i] = 1;
            continue;
        }
        const i64 start = a.run_start[g];
        const i64 place = i - start + 1;   // the row number
        i64 value = place;
        if (a.peer_flag) {
            // the peer run of row i: the flags before it, plus its own, minus one
            const i32 p = a.peer_index[i] + a.peer_flag[i] - 1;
            value = (i64)a.peer_start[p] - start + 1;
        }
        a.ranking[i] = value;
        a.keep[i] = value <= a.limit ? (u8)1 : (u8)0;
        // place n of the run: for ROW_NUMBER the last row kept; for RANK a row whose rank is <= n and whose peers, the last row kept
        // among them, share its image
        if (place == a.limit && g < (u64)a.bound_n) a.bound[g] = a.images[a.perm[i]];
    }
}

inline int grid_of(int64_t work)
{
    int64_t g = (work + 255) / 256;
    if (g < 1) g = 1;
    if (g > 256 * 16) g = 256 * 16;
    return (int)g;
}

}  // namespace

void launch_topn_ranking_filter(const uint64_t* gids, const uint64_t* images, const uint64_t* bound, int64_t bound_n, int32_t n, uint8_t* keep, hipStream_t s)
{
    if (n <= 0) return;
    const int blocks = (int)(((int64_t)n + kTopNRankingRowsPerBlock - 1) / kTopNRankingRowsPerBlock);
    hipLaunchKernelGGL(k_topn_ranking_filter, blocks, 256, 0, s, (const u64*)gids, (const u64*)images, (const u64*)bound, (i64)bound_n, n, keep);
    PA_HIP(hipGetLastError());
}

void launch_topn_ranking_differs(int32_t type, const void* values, const int32_t* offsets, const uint8_t* nulls, const int32_t* perm, int32_t n,
                                 uint8_t* differs, hipStream_t s)
{
    if (n <= 1) return;
    hipLaunchKernelGGL(k_topn_ranking_differs, grid_of(n), 256, 0, s, type, values, offsets, nulls, perm, n, differs);
    PA_HIP(hipGetLastError());
}

void launch_topn_ranking_heads(const uint64_t* sorted_gids, const uint8_t* differs, int32_t n, int32_t* run_start, int64_t run_start_n, int32_t* peer_flag,
                               hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_topn_ranking_heads, grid_of(n), 256, 0, s, (const u64*)sorted_gids, differs, n, run_start, (i64)run_start_n, peer_flag);
    PA_HIP(hipGetLastError());
}

void launch_topn_ranking_peer_starts(const int32_t* peer_flag, const int32_t* peer_index, int32_t n, int32_t* peer_start, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_topn_ranking_peer_starts, grid_of(n), 256, 0, s, peer_flag, peer_index, n, peer_start);
    PA_HIP(hipGetLastError());
}

void launch_topn_ranking_rank(const TopNRankingRankArgs& a, hipStream_t s)
{
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_topn_ranking_rank, grid_of(a.n), 256, 0, s, a);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
