// window_kernels.hip -- the passes of WindowOperator behind its sort (window_kernels.hpp).
#include <hip/hip_runtime.h>

#include "window_kernels.hpp"
#include "kernels/pa_row_distinct.h"

namespace pa {

namespace {

// IS DISTINCT FROM the sorted row before, per channel (not the comparator's rule, under which -0.0 differs from +0.0)
__global__ __launch_bounds__(256) void k_window_distinct(i32 type, const void* __restrict__ values, const i32* __restrict__ offsets, const u8* __restrict__ nulls,
                                                         const i32* __restrict__ perm, i32 n, i32* __restrict__ flag_a, i32* __restrict__ flag_b)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x + 1; i < n; i += (i64)gridDim.x * 256) {
        if (!row_distinct<true>(type, values, offsets, nulls, perm[i - 1], perm[i])) continue;
        flag_a[i] = 1;
        if (flag_b) flag_b[i] = 1;
    }
}

__global__ __launch_bounds__(256) void k_window_starts(const i32* __restrict__ part_flag, const i32* __restrict__ part_index, const i32* __restrict__ peer_flag,
                                                       const i32* __restrict__ peer_index, i32 n, i32* __restrict__ part_start, i32* __restrict__ peer_start)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const i32 pf = part_flag[i], qf = peer_flag[i];
        const i32 p = part_index[i] + pf, q = peer_index[i] + qf;   // both in [0, i]
        if (i == 0 || pf) part_start[p] = (i32)i;
        if (i == 0 || qf) peer_start[q] = (i32)i;
        if (i == n - 1) {   // the sentinel behind the last run: p + 1, q + 1 <= n
            part_start[p + 1] = n;
            peer_start[q + 1] = n;
        }
    }
}

// NTileFunction.bucket in int64: place i of a partition of N rows
__device__ __forceinline__ i64 ntile_bucket(i64 i, i64 N, i64 buckets)
{
    if (N < buckets) return i;
    const i64 r = N % buckets, q = N / buckets;
    return i < (q + 1) * r ? i / (q + 1) : (i - r) / q;
}

// A workgroup takes 1024 consecutive sorted rows, a lane four of them 256 apart: every load and store of a wave is one contiguous run,
// and the four rows' dependent reads (index -> start) are in flight together.  The function ids are the same in every lane.
__global__ __launch_bounds__(256) void k_window_functions(WindowFunctionArgs a)
{
    const i32 n = a.n;
    const i64 base = (i64)blockIdx.x * kWindowRowsPerBlock + threadIdx.x;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const i64 i = base + 256 * e;
        if (i >= n) continue;
        const i32 p = a.part_index[i] + a.part_flag[i], q = a.peer_index[i] + a.peer_flag[i];
        i64 first = a.part_start[p];
        first = first < 0 ? 0 : first > i ? i : first;   // (first <= i by construction: never an index outside the arrays)
        const i64 N = (i64)a.part_start[p + 1] - first;           // rows of the partition
        const i64 place = i - first;                              // 0-based
        const i64 ps = (i64)a.peer_start[q] - first;              // the peer group's places [ps, pe)
        const i64 pe = (i64)a.peer_start[q + 1] - first;
        const i64 d = (i64)q - (i64)(a.peer_index[first] + a.peer_flag[first]) + 1;   // peer groups up to and including its own
        for (int k = 0; k < a.count; k++) {
            const WindowFunction& f = a.f[k];
            switch (f.function) {
                case PA_WINDOW_ROW_NUMBER: ((i64*)f.out)[i] = place + 1; break;
                case PA_WINDOW_RANK: ((i64*)f.out)[i] = ps + 1; break;
                case PA_WINDOW_DENSE_RANK: ((i64*)f.out)[i] = d; break;
                case PA_WINDOW_PERCENT_RANK: ((double*)f.out)[i] = N == 1 ? 0.0 : (double)ps / (double)(N - 1); break;
                case PA_WINDOW_CUME_DIST: ((double*)f.out)[i] = (double)pe / (double)N; break;
                case PA_WINDOW_NTILE: {
                    const i64 row = a.perm[i];
                    const bool is_null = f.arg_nulls && f.arg_nulls[row];
                    i64 value = 0;
                    if (!is_null) {
                        const i64 buckets = f.arg_type == PA_BIGINT ? ((const i64*)f.arg_values)[row] : (i64)((const i32*)f.arg_values)[row];
                        if (buckets <= 0) atomicOr(a.error, 1);
                        else value = ntile_bucket(place, N, buckets) + 1;
                    }
                    ((i64*)f.out)[i] = value;
                    if (f.out_nulls) f.out_nulls[i] = is_null ? (u8)1 : (u8)0;
                    break;
                }
                default: break;
            }
        }
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

void launch_window_distinct(int32_t type, const void* values, const int32_t* offsets, const uint8_t* nulls, const int32_t* perm, int32_t n,
                            int32_t* flag_a, int32_t* flag_b, hipStream_t s)
{
    if (n <= 1) return;
    hipLaunchKernelGGL(k_window_distinct, grid_of(n), 256, 0, s, type, values, offsets, nulls, perm, n, flag_a, flag_b);
    PA_HIP(hipGetLastError());
}

void launch_window_starts(const int32_t* part_flag, const int32_t* part_index, const int32_t* peer_flag, const int32_t* peer_index, int32_t n,
                          int32_t* part_start, int32_t* peer_start, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_window_starts, grid_of(n), 256, 0, s, part_flag, part_index, peer_flag, peer_index, n, part_start, peer_start);
    PA_HIP(hipGetLastError());
}

void launch_window_functions(const WindowFunctionArgs& a, hipStream_t s)
{
    if (a.n <= 0 || a.count <= 0) return;
    const int blocks = (int)(((int64_t)a.n + kWindowRowsPerBlock - 1) / kWindowRowsPerBlock);
    hipLaunchKernelGGL(k_window_functions, blocks, 256, 0, s, a);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
