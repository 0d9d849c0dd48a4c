// pa_row_distinct.h -- do two rows of one channel hold different values?  The one comparison behind the run-detection kernels
// (k_window_distinct, k_topn_ranking_differs): two NULLs are the same value, a NULL differs from every value.
//   zeros_equal = true    IS DISTINCT FROM: -0.0 equals +0.0, NaN equals NaN (Window's partitions and peer groups)
//   zeros_equal = false   the comparator's identity (Double.compare): all NaNs are one value, -0.0 and +0.0 are two (TopNRanking's peers)
#pragma once

#include "pa_device.h"

namespace pa {

__device__ __forceinline__ u64 value_bits(double d) { return (u64)__double_as_longlong(d); }
__device__ __forceinline__ u64 value_bits(float f) { return (u32)__float_as_int(f); }

template <bool zeros_equal, typename F>
__device__ __forceinline__ bool float_distinct(F x, F y)
{
    if (x != x || y != y) return (x != x) != (y != y);   // a NaN: distinct from everything but a NaN
    return zeros_equal ? x != y : value_bits(x) != value_bits(y);
}

template <bool zeros_equal>
__device__ __forceinline__ bool row_distinct(i32 type, const void* __restrict__ values, const i32* __restrict__ offsets, const u8* __restrict__ nulls, i64 a, i64 b)
{
    const bool na = nulls && nulls[a], nb = nulls && nulls[b];
    if (na || nb) return na != nb;
    switch (type) {
        case PA_BIGINT:
        case PA_DECIMAL: return ((const i64*)values)[a] != ((const i64*)values)[b];
        case PA_INTEGER:
        case PA_DATE: return ((const i32*)values)[a] != ((const i32*)values)[b];
        case PA_BOOLEAN: return (((const u8*)values)[a] != 0) != (((const u8*)values)[b] != 0);
        case PA_DOUBLE: return float_distinct<zeros_equal>(((const double*)values)[a], ((const double*)values)[b]);
        case PA_REAL: return float_distinct<zeros_equal>(((const float*)values)[a], ((const float*)values)[b]);
        case PA_VARCHAR: {
            const i32 oa = offsets[a], ob = offsets[b], la = offsets[a + 1] - oa, lb = offsets[b + 1] - ob;
            if (la != lb) return true;
            const u8* pa_ = (const u8*)values + oa;
            const u8* pb_ = (const u8*)values + ob;
            for (i32 j = 0; j < la; j++)
                if (pa_[j] != pb_[j]) return true;
            return false;
        }
        default: return true;
    }
}

}  // namespace pa
