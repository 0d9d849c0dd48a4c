// semi_join_kernels.hip -- HashSemiJoinOperator's mark on device (HashSemiJoinOperator.java:168-221).
//
// The set is a lookup source of the join build (op_join.cpp) over one channel; for every probe row ONE pass writes the mark and
// its NULL flag -- no count pass, no scan, no position lists, no gathers.  A lane takes four consecutive rows: the key column is
// read in 32-byte runs per lane (coalesced across the wave) and the marks go out as one 4-byte word per lane instead of four byte
// stores.  One specialisation per layout of the lookup source (SemiLayout), picked on the host.
#include <hip/hip_runtime.h>

#include "semi_join_kernels.hpp"
#include "kernels/pa_device.h"
#include "kernels/pa_canon.h"

namespace pa {

static inline int semi_grid(int64_t work)
{
    int64_t g = (work + 255) / 256;
    if (g < 1) g = 1;
    if (g > 256 * 16) g = 256 * 16;
    return (int)g;
}

__global__ __launch_bounds__(256) void k_semi_canon(JoinCol key, i32 n, u64* __restrict__ out, i32* __restrict__ any_null)
{
    const i64 padded = ((i64)n + 63) & ~(i64)63;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < padded; i += (i64)gridDim.x * 256) {
        bool null = false;
        if (i < n) {
            null = key.nulls != nullptr && key.nulls[i] != 0;
            out[i] = null ? 0ULL : semi_canon_bits(key.type, key.values, i);
        }
        if (__ballot(null) != 0ULL && (threadIdx.x & 63) == 0) *any_null = 1;
    }
}

__global__ __launch_bounds__(256) void k_semi_any_null(const u8* __restrict__ nulls, i32 n, i32* __restrict__ any_null)
{
    const i64 padded = ((i64)n + 63) & ~(i64)63;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < padded; i += (i64)gridDim.x * 256) {
        const bool null = i < n && nulls[i] != 0;
        if (__ballot(null) != 0ULL && (threadIdx.x & 63) == 0) *any_null = 1;
    }
}

// presence of a canonical key in the keyed slot table (k_join_probe_count_keyed's sequence: a 64-byte line of 4 slots per trip)
__device__ __forceinline__ bool semi_in_slots(const JoinKeySlot* __restrict__ slots, u32 mask, u32 wrap, u64 v)
{
    u32 pos = (u32)pa_murmur3_fmix((u64)pa_hash_bigint((i64)v)) & mask;
    const uint4* lines = (const uint4*)slots;
    for (u32 seen = 0; seen <= wrap;) {
        const u32 base = pos & ~3u, first = pos & 3u;
        uint4 q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = lines[base + k];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((u32)k < first) continue;
            if ((i32)q[k].z == -1) return false;
            if ((((u64)q[k].y << 32) | (u64)q[k].x) == v) return true;
        }
        seen += 4u - first;
        pos = (pos & ~wrap) | ((base + 4u) & wrap);
    }
    return false;
}

// presence of a VARCHAR value in the tagged table of the generic build (k_join_probe_count's sequence), byte equality
__device__ __forceinline__ bool semi_in_tagged(const u64* __restrict__ tagged, u32 mask, const JoinCol& build, const JoinCol& probe, i64 r, i64 raw)
{
    const u64 mixed = (u64)pa_murmur3_fmix((u64)raw);
    u32 pos = (u32)mixed & mask;
    const ulonglong2* lines = (const ulonglong2*)tagged;
    const i32 po = probe.offsets[r];
    const i32 plen = probe.offsets[r + 1] - po;
    const u8* pv = (const u8*)probe.values + po;
    for (u32 seen = 0; seen <= mask;) {
        const u32 base = pos & ~7u, first = pos & 7u;
        ulonglong2 q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = lines[(base >> 1) + k];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if ((u32)k < first) continue;
            const u64 t = (k & 1) ? q[k >> 1].y : q[k >> 1].x;
            const i32 cur = (i32)(u32)t;
            if (cur == -1) return false;
            if (((t ^ mixed) >> 32) == 0ULL) {
                const i32 bo = build.offsets[cur];
                if (pa_str_eq((const u8*)build.values + bo, build.offsets[cur + 1] - bo, pv, plen)) return true;
            }
        }
        seen += 8u - first;
        pos = (base + 8u) & mask;
    }
    return false;
}

// kVec: an 8-byte key column at a 16-byte aligned address -- a lane's four keys come in as two 16-byte loads
template <int kLayout, bool kVec>
__global__ __launch_bounds__(256) void k_semi_mark(SemiProbeArgs a)
{
    const i64 quads = ((i64)a.n + 3) >> 2;
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < quads; q += (i64)gridDim.x * 256) {
        const i64 r0 = 4 * q;
        u64 k[4];
        bool live[4];
#pragma unroll
        for (int j = 0; j < 4; j++) live[j] = r0 + j < a.n && !(a.key.nulls != nullptr && a.key.nulls[r0 + j] != 0);
        if (kLayout != SEMI_TAGGED && kLayout != SEMI_EMPTY) {
            if (kVec && r0 + 3 < a.n) {
                const ulonglong2* p = (const ulonglong2*)((const u64*)a.key.values + r0);
                const ulonglong2 lo = p[0], hi = p[1];
                k[0] = lo.x;
                k[1] = lo.y;
                k[2] = hi.x;
                k[3] = hi.y;
                if (a.key.type == PA_DOUBLE) {
#pragma unroll
                    for (int j = 0; j < 4; j++) k[j] = semi_canon_bits(PA_DOUBLE, &k[j], 0);
                }
            }
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) k[j] = r0 + j < a.n ? semi_canon_bits(a.key.type, a.key.values, r0 + j) : 0ULL;
            }
        }
        u32 mark = 0, null = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (r0 + j >= a.n) continue;
            bool hit = false;
            if (live[j]) {
                if (kLayout == SEMI_BITMAP) {
                    const u64 d = (u64)((i64)k[j] - a.bitmap.min_key);
                    hit = d <= a.bitmap.range && ((a.bitmap.bits[d >> 6] >> (d & 63ULL)) & 1ULL) != 0ULL;
                }
                else if (kLayout == SEMI_SLOTS) hit = semi_in_slots(a.slots, a.mask, a.wrap, k[j]);
                else if (kLayout == SEMI_TAGGED) hit = semi_in_tagged((const u64*)a.tagged, a.mask, a.build_key, a.key, r0 + j, a.probe_hash[r0 + j]);
            }
            // HashSemiJoinOperator.java:190-218
            const bool is_null = live[j] ? (!hit && a.miss_is_null) : (a.null_is_null != 0);
            mark |= (hit ? 1u : 0u) << (8 * j);
            null |= (is_null ? 1u : 0u) << (8 * j);
        }
        ((u32*)a.mark)[q] = mark;
        if (a.mark_null) {
            ((u32*)a.mark_null)[q] = null;
            if (__ballot(null != 0) != 0ULL && (threadIdx.x & 63) == 0) *a.any_null_mark = 1;
        }
    }
}

void launch_semi_canon(const JoinCol& key, int32_t n, uint64_t* out, int32_t* any_null, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_semi_canon, semi_grid(n), 256, 0, s, key, n, (u64*)out, any_null);
    PA_HIP(hipGetLastError());
}
void launch_semi_any_null(const uint8_t* nulls, int32_t n, int32_t* any_null, hipStream_t s)
{
    if (n <= 0 || nulls == nullptr) return;
    hipLaunchKernelGGL(k_semi_any_null, semi_grid(n), 256, 0, s, nulls, n, any_null);
    PA_HIP(hipGetLastError());
}

template <int kLayout>
static const char* launch_layout(const SemiProbeArgs& a, bool vec, const char* name, hipStream_t s)
{
    const int grid = semi_grid(((int64_t)a.n + 3) / 4);
    if (vec) hipLaunchKernelGGL((k_semi_mark<kLayout, true>), grid, 256, 0, s, a);
    else hipLaunchKernelGGL((k_semi_mark<kLayout, false>), grid, 256, 0, s, a);
    PA_HIP(hipGetLastError());
    return name;
}
const char* launch_semi_mark(const SemiProbeArgs& a, hipStream_t s)
{
    if (a.n <= 0) return "";
    const bool wide = a.key.type == PA_BIGINT || a.key.type == PA_DECIMAL || a.key.type == PA_DOUBLE;
    const bool vec = wide && ((uintptr_t)a.key.values & 15u) == 0;
    switch (a.layout) {
        case SEMI_BITMAP: return launch_layout<SEMI_BITMAP>(a, vec, "k_semi_mark_bitmap", s);
        case SEMI_SLOTS: return launch_layout<SEMI_SLOTS>(a, vec, "k_semi_mark_slots", s);
        case SEMI_TAGGED: return launch_layout<SEMI_TAGGED>(a, false, "k_semi_mark_tagged", s);
        default: return launch_layout<SEMI_EMPTY>(a, false, "k_semi_mark_empty", s);
    }
}

__device__ __forceinline__ void semi_count_add(u64 mine, unsigned long long* out)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine != 0) atomicAdd(out, (unsigned long long)mine);
}
__global__ __launch_bounds__(256) void k_semi_count_bits(const u64* __restrict__ words, i64 nwords, unsigned long long* out)
{
    u64 mine = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (i64)gridDim.x * 256) mine += (u64)__popcll(words[i]);
    semi_count_add(mine, out);
}
__global__ __launch_bounds__(256) void k_semi_count_slots(const JoinKeySlot* __restrict__ slots, i64 size, unsigned long long* out)
{
    u64 mine = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < size; i += (i64)gridDim.x * 256) mine += slots[i].head != -1 ? 1 : 0;
    semi_count_add(mine, out);
}
__global__ __launch_bounds__(256) void k_semi_count_tagged(const u64* __restrict__ tagged, i64 size, unsigned long long* out)
{
    u64 mine = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < size; i += (i64)gridDim.x * 256) mine += tagged[i] != ~0ULL ? 1 : 0;
    semi_count_add(mine, out);
}
void launch_semi_count_bits(const uint64_t* words, int64_t nwords, unsigned long long* out, hipStream_t s)
{
    if (nwords <= 0) return;
    hipLaunchKernelGGL(k_semi_count_bits, semi_grid(nwords), 256, 0, s, (const u64*)words, nwords, out);
    PA_HIP(hipGetLastError());
}
void launch_semi_count_slots(const JoinKeySlot* slots, int64_t size, unsigned long long* out, hipStream_t s)
{
    if (size <= 0) return;
    hipLaunchKernelGGL(k_semi_count_slots, semi_grid(size), 256, 0, s, slots, size, out);
    PA_HIP(hipGetLastError());
}
void launch_semi_count_tagged(const uint64_t* tagged, int64_t size, unsigned long long* out, hipStream_t s)
{
    if (size <= 0) return;
    hipLaunchKernelGGL(k_semi_count_tagged, semi_grid(size), 256, 0, s, (const u64*)tagged, size, out);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
