// nested_loop_kernels.hpp -- what the NestedLoopJoin operator (op_nested_loop.cpp) shares with its kernels: the launcher of the
// static position kernel (nested_loop_kernels.hip) and the constants of the generated pair kernels.
#pragma once

#include "common.hpp"

namespace pa {

// Variant 0 of the generated pair kernels (lanes over probe rows) stages the build's filter channels through LDS this many build
// rows at a time; every lane of the workgroup then reads build row jj of the chunk at one address (a broadcast).
constexpr int kNestedLoopLdsChunk = 1024;
// ... when one chunk of all of them fits into this much LDS (3 workgroups of 256 threads per CU); else they are read from memory
constexpr int kNestedLoopLdsBytes = 48 << 10;
// (channels of the build page and the probe page together: PA_NL_MAX_CHANNELS, with the pair kernels' argument block in kernels/pa_args.h)

// The plain product of the probe rows [i0, i0 + n) with the build rows [j0, j0 + m), probe-major: for t in [0, n * m)
// probe_idx[t] = i0 + t / m, build_pos[t] = j0 + t % m.  n * m < 2^31.
void launch_nested_loop_product(int32_t i0, int32_t n, int32_t j0, int32_t m, int32_t* probe_idx, int32_t* build_pos, hipStream_t s);

}  // namespace pa
