// unique_id_kernels.hip -- the id column of AssignUniqueIdOperator (unique_id_kernels.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "unique_id_kernels.hpp"
#include "kernels/pa_device.h"

namespace pa {

// A lane takes rows begin + lane, begin + lane + grid, ...: consecutive lanes store consecutive 8-byte words.  The segment of a row is
// found by walking the (at most eight) segment starts; they sit in the kernel arguments and are only ever indexed by the unrolled
// loop's constant, so they stay in scalar registers.  Slots behind a.segments hold first_row = INT32_MAX and never match.
__global__ __launch_bounds__(256) void k_unique_ids(UniqueIdArgs a, i64 end)
{
    for (i64 i = a.first_row[0] + (i64)blockIdx.x * 256 + threadIdx.x; i < end; i += (i64)gridDim.x * 256) {
        i64 row0 = a.first_row[0], id0 = a.first_id[0];
#pragma unroll
        for (int j = 1; j < kUniqueIdSegments; j++) {
            if (i >= a.first_row[j]) {
                row0 = a.first_row[j];
                id0 = a.first_id[j];
            }
        }
        a.ids[i] = id0 + (i - row0);
    }
}

void launch_unique_ids(const UniqueIdArgs& args, hipStream_t s)
{
    UniqueIdArgs a = args;
    PA_REQUIRE(a.ids != nullptr && a.segments >= 1 && a.segments <= kUniqueIdSegments, PA_ERR_DEVICE, "unique ids: segment count out of range");
    int64_t rows = 0;
    for (int k = 0; k < a.segments; k++) {
        PA_REQUIRE(a.rows[k] > 0 && a.first_row[k] >= 0 && (k == 0 || a.first_row[k] == a.first_row[k - 1] + a.rows[k - 1]), PA_ERR_DEVICE,
                   "unique ids: segments do not follow each other");
        rows += a.rows[k];
    }
    const int64_t end = a.first_row[0] + rows;
    PA_REQUIRE(end <= INT32_MAX, PA_ERR_DEVICE, "unique ids: rows beyond a page");
    for (int k = a.segments; k < kUniqueIdSegments; k++) {
        a.first_row[k] = INT32_MAX;
        a.rows[k] = 0;
        a.first_id[k] = 0;
    }
    const int64_t blocks = (rows + 255) / 256;
    const int grid = (int)std::min<int64_t>(blocks, (int64_t)device_cu_count() * 8);
    hipLaunchKernelGGL(k_unique_ids, grid, 256, 0, s, a, (i64)end);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
