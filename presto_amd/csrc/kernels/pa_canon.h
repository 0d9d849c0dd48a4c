// pa_canon.h -- the canonical 64-bit key of a value under IS NOT DISTINCT FROM, shared by the statically compiled kernels that
// compare keys as integers (semi_join_kernels.hip, distinct_kernels.hip).  Needs pa_device.h and the PA_* type codes.
#pragma once

// IS NOT DISTINCT FROM as equality of 64-bit keys (semi_join_kernels.hpp)
__device__ __forceinline__ u64 semi_canon_bits(i32 type, const void* values, i64 r)
{
    switch (type) {
        case PA_INTEGER:
        case PA_DATE: return (u64)(i64)((const i32*)values)[r];
        case PA_BOOLEAN: return ((const u8*)values)[r] != 0 ? 1ULL : 0ULL;  // any non-zero byte is true
        case PA_DOUBLE: {
            const u64 b = ((const u64*)values)[r];
            if ((b & 0x7fffffffffffffffULL) > 0x7ff0000000000000ULL) return 0x7ff8000000000000ULL;  // every NaN is one value (DoubleType.java:181-192)
            return b == 0x8000000000000000ULL ? 0ULL : b;                                            // -0.0 is +0.0
        }
        case PA_REAL: {
            const u32 b = ((const u32*)values)[r];
            if ((b & 0x7fffffffu) > 0x7f800000u) return 0x7fc00000ULL;
            return b == 0x80000000u ? 0ULL : (u64)b;
        }
        default: return ((const u64*)values)[r];  // BIGINT, short DECIMAL (the unscaled value)
    }
}
