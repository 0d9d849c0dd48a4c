// nested_loop_kernels.hip -- the position lists of a NestedLoopJoin without a filter: arithmetic, no input read.
// (The kernels of a join WITH a filter are generated per plan: op_nested_loop.cpp.)
#include <hip/hip_runtime.h>

#include "nested_loop_kernels.hpp"
#include "kernels/pa_device.h"

namespace pa {

// A lane writes four consecutive pairs as two 16-byte stores; the division by m is one per lane, the three pairs behind it step.
__global__ __launch_bounds__(256) void k_nested_loop_product(i32 i0, i32 j0, u32 m, i64 total, i32* __restrict__ probe_idx, i32* __restrict__ build_pos)
{
    const i64 quads = (total + 3) >> 2;
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < quads; q += (i64)gridDim.x * 256) {
        const i64 t = q << 2;
        u32 i = (u32)((u64)t / m), j = (u32)((u64)t - (u64)i * m);
        i32 p[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            p[r] = i0 + (i32)i;
            b[r] = j0 + (i32)j;
            if (++j == m) {
                j = 0;
                i++;
            }
        }
        if (t + 4 <= total) {
            ((pa_i32x4*)probe_idx)[q] = pa_i32x4{p[0], p[1], p[2], p[3]};
            ((pa_i32x4*)build_pos)[q] = pa_i32x4{b[0], b[1], b[2], b[3]};
        }
        else {
            for (int r = 0; t + r < total; r++) {
                probe_idx[t + r] = p[r];
                build_pos[t + r] = b[r];
            }
        }
    }
}

void launch_nested_loop_product(int32_t i0, int32_t n, int32_t j0, int32_t m, int32_t* probe_idx, int32_t* build_pos, hipStream_t s)
{
    const int64_t total = (int64_t)n * m;
    if (total <= 0) return;
    int64_t grid = ((total + 3) / 4 + 255) / 256;
    if (grid > 256 * 16) grid = 256 * 16;
    hipLaunchKernelGGL(k_nested_loop_product, (int)grid, 256, 0, s, (i32)i0, (i32)j0, (u32)m, (i64)total, probe_idx, build_pos);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
