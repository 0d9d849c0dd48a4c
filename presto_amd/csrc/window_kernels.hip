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

// ---- the aggregates: gather, segmented scans ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window_gather(i32 type, const void* __restrict__ values, const u8* __restrict__ nulls, const i32* __restrict__ perm, i32 n,
                                                       u64* __restrict__ sorted_values, u8* __restrict__ sorted_nulls)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const i64 row = perm[i];
        if (sorted_nulls) sorted_nulls[i] = nulls[row] ? (u8)1 : (u8)0;
        if (!sorted_values) continue;
        u64 v;
        switch (type) {
            case PA_INTEGER:
            case PA_DATE: v = (u64)(i64)((const i32*)values)[row]; break;
            case PA_BOOLEAN: v = ((const u8*)values)[row] ? 1ULL : 0ULL; break;
            case PA_REAL: v = (u64)__double_as_longlong((double)((const float*)values)[row]); break;
            default: v = ((const u64*)values)[row]; break;   // BIGINT, short DECIMAL, DOUBLE
        }
        sorted_values[i] = v;
    }
}

// The state of a scan with the flag "a partition starts here or before, inside what this state covers".  count: b = the non-null rows;
// sum: (b, a) = the 96-bit sum, a its low word (n <= INT32_MAX values of 64 bits: exact); min / max: a = the held value, b = there is one.
struct WindowAcc {
    u64 a;
    i32 b;
    i32 f;
};
// how min / max compare: the key of a value under the mode; the held value is replaced when the new key is smaller (min) / greater (max)
enum { kCmpInt = 0, kCmpDoubleMin = 1, kCmpDoubleMax = 2 };
__device__ __forceinline__ i64 minmax_key(u64 bits, int mode)
{
    if (mode == kCmpInt) return (i64)bits;
    const bool nan = (bits & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL;
    const i64 b = (i64)bits;
    const i64 image = b < 0 ? (b ^ 0x7FFFFFFFFFFFFFFFLL) : b;   // Double.compare order of the non-NaN values: -0.0 -> -1, +0.0 -> 0
    if (mode == kCmpDoubleMin) return nan ? 0x7FFFFFFFFFFFFFFFLL : image;   // NaN largest
    return nan ? (i64)0x8000000000000000ULL : (image == -1 ? 0 : image);    // max: NaN loses to everything (-inf included), the zeros tie
}
// x (f1, v1) before y (f2, v2): (f1 | f2, f2 ? v2 : v1 + v2)
template <int KIND>
__device__ __forceinline__ WindowAcc acc_combine(WindowAcc x, WindowAcc y, int mode)
{
    // (selects field by field, no early return: a choice between two structs would leave them in scratch)
    const bool restart = y.f != 0;
    WindowAcc r;
    r.f = x.f | y.f;
    if (KIND == kWindowScanCount) {
        r.a = 0;
        r.b = restart ? y.b : x.b + y.b;
    }
    else if (KIND == kWindowScanSum) {
        const u64 lo = x.a + y.a;
        r.a = restart ? y.a : lo;
        r.b = restart ? y.b : x.b + y.b + (lo < x.a ? 1 : 0);
    }
    else {
        const i64 kx = minmax_key(x.a, mode), ky = minmax_key(y.a, mode);
        const bool better = KIND == kWindowScanMin ? ky < kx : ky > kx;
        // keep the left unless there is none or the right is strictly better
        const bool take = restart || !x.b || (y.b && better);
        r.a = take ? y.a : x.a;
        r.b = take ? y.b : x.b;
    }
    return r;
}
template <int KIND>
__device__ __forceinline__ WindowAcc acc_shfl_up(const WindowAcc& v, int off)
{
    WindowAcc o;
    o.a = KIND == kWindowScanCount ? 0 : (u64)__shfl_up((long long)v.a, off, 64);
    o.b = __shfl_up(v.b, off, 64);
    o.f = __shfl_up(v.f, off, 64);
    return o;
}
__device__ __forceinline__ WindowAcc acc_identity()
{
    WindowAcc r;
    r.a = 0;
    r.b = 0;
    r.f = 0;
    return r;
}

// The four consecutive entries of a lane, combined in place (s[j] = e[0] + ... + e[j]), then over the 256 lanes of the workgroup: the
// state of everything in front of the lane's entries inside the workgroup (returned) and of the whole workgroup (*total).
template <int KIND>
__device__ __forceinline__ WindowAcc acc_block_scan(WindowAcc (&s)[4], int mode, WindowAcc* total)
{
    __shared__ WindowAcc wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 1; j < 4; j++) s[j] = acc_combine<KIND>(s[j - 1], s[j], mode);
    WindowAcc inc = s[3];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const WindowAcc o = acc_shfl_up<KIND>(inc, off);
        if (lane >= off) inc = acc_combine<KIND>(o, inc, mode);
    }
    if (lane == 63) wave_total[wave] = inc;
    WindowAcc before = acc_shfl_up<KIND>(inc, 1);
    if (lane == 0) before = acc_identity();
    __syncthreads();
    WindowAcc front = acc_identity(), all = acc_identity();
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const WindowAcc t = wave_total[w];
        if (w < wave) front = acc_combine<KIND>(front, t, mode);
        all = acc_combine<KIND>(all, t, mode);
    }
    __syncthreads();
    *total = all;
    return acc_combine<KIND>(front, before, mode);
}

// the entries of sorted rows base .. base + 3 (rows at or past n: the identity)
template <int KIND>
__device__ __forceinline__ void acc_load_rows(WindowAcc (&s)[4], i64 base, i32 n, const u64* __restrict__ values, const u8* __restrict__ nulls,
                                              const i32* __restrict__ part_flag)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const i64 i = base + j;
        s[j] = acc_identity();
        if (i >= n) continue;
        const bool is_null = nulls && nulls[i];
        s[j].f = part_flag[i];
        if (KIND == kWindowScanCount) s[j].b = is_null ? 0 : 1;
        else if (KIND == kWindowScanSum) {
            const i64 v = is_null ? 0 : (i64)values[i];
            s[j].a = (u64)v;
            s[j].b = v < 0 ? -1 : 0;
        }
        else {
            s[j].a = values[i];
            s[j].b = is_null ? 0 : 1;
        }
    }
}

// launch 1 of 3: the state of every tile of kWindowScanTile rows
template <int KIND>
__global__ __launch_bounds__(256) void k_window_scan_tiles(const u64* __restrict__ values, const u8* __restrict__ nulls, const i32* __restrict__ part_flag, i32 n,
                                                           int mode, WindowAcc* __restrict__ tile_acc)
{
    WindowAcc s[4], total;
    acc_load_rows<KIND>(s, (i64)blockIdx.x * kWindowScanTile + (i64)threadIdx.x * 4, n, values, nulls, part_flag);
    (void)acc_block_scan<KIND>(s, mode, &total);
    if (threadIdx.x == 0) tile_acc[blockIdx.x] = total;
}

// launch 2 of 3, one workgroup: tile_front[t] = the state of the tiles in front of tile t, kWindowScanTile tiles at a time
template <int KIND>
__global__ __launch_bounds__(256) void k_window_scan_tile_fronts(const WindowAcc* __restrict__ tile_acc, i32 tiles, int mode, WindowAcc* __restrict__ tile_front)
{
    WindowAcc carry = acc_identity();
    for (i32 chunk = 0; chunk < tiles; chunk += kWindowScanTile) {
        const i32 base = chunk + (i32)threadIdx.x * 4;
        WindowAcc e[4], s[4], total;
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = e[j] = base + j < tiles ? tile_acc[base + j] : acc_identity();
        WindowAcc front = acc_combine<KIND>(carry, acc_block_scan<KIND>(s, mode, &total), mode);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (base + j < tiles) tile_front[base + j] = front;
            front = acc_combine<KIND>(front, e[j], mode);
        }
        carry = acc_combine<KIND>(carry, total, mode);
    }
}

// launch 3 of 3: the tile's own scan behind the state in front of it; a prefix sum outside int64 sets its bit of the error word
template <int KIND>
__global__ __launch_bounds__(256) void k_window_scan_apply(const u64* __restrict__ values, const u8* __restrict__ nulls, const i32* __restrict__ part_flag, i32 n,
                                                           int mode, const WindowAcc* __restrict__ tile_front, void* __restrict__ out, i32* __restrict__ error)
{
    const i64 base = (i64)blockIdx.x * kWindowScanTile + (i64)threadIdx.x * 4;
    WindowAcc s[4], total;
    acc_load_rows<KIND>(s, base, n, values, nulls, part_flag);
    const WindowAcc front = acc_combine<KIND>(tile_front[blockIdx.x], acc_block_scan<KIND>(s, mode, &total), mode);
    bool overflow = false;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const i64 i = base + j;
        if (i >= n) continue;
        const WindowAcc r = acc_combine<KIND>(front, s[j], mode);
        if (KIND == kWindowScanCount) ((i32*)out)[i] = r.b;
        else ((u64*)out)[i] = r.a;
        if (KIND == kWindowScanSum && r.b != ((i64)r.a < 0 ? -1 : 0)) overflow = true;
    }
    if (KIND == kWindowScanSum && overflow) atomicOr(error, kWindowErrorSum);
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
                        if (buckets <= 0) atomicOr(a.error, kWindowErrorBuckets);
                        else value = ntile_bucket(place, N, buckets) + 1;
                    }
                    ((i64*)f.out)[i] = value;
                    if (f.out_nulls) f.out_nulls[i] = is_null ? (u8)1 : (u8)0;
                    break;
                }
                case PA_WINDOW_COUNT_STAR:
                case PA_WINDOW_COUNT:
                case PA_WINDOW_SUM:
                case PA_WINDOW_MIN:
                case PA_WINDOW_MAX: {
                    // the frame is places 0 .. e; its state stands at sorted row first + e, inside [i, n)
                    const i64 e = f.frame_end == kWindowFrameRow ? place : f.frame_end == kWindowFramePeers ? pe - 1 : N - 1;
                    i64 at = first + e;
                    at = at < i ? i : at > (i64)n - 1 ? (i64)n - 1 : at;
                    const i64 rows = f.count ? (i64)f.count[at] : e + 1;   // the frame's non-null rows
                    if (f.function == PA_WINDOW_COUNT_STAR) ((i64*)f.out)[i] = e + 1;
                    else if (f.function == PA_WINDOW_COUNT) ((i64*)f.out)[i] = rows;
                    else {
                        const u64 v = rows > 0 ? ((const u64*)f.scan)[at] : 0ULL;
                        if (f.function == PA_WINDOW_SUM) ((u64*)f.out)[i] = v;
                        else switch (f.arg_type) {
                            case PA_INTEGER:
                            case PA_DATE: ((i32*)f.out)[i] = (i32)(i64)v; break;
                            case PA_REAL: ((float*)f.out)[i] = (float)__longlong_as_double((long long)v); break;
                            case PA_BOOLEAN: ((u8*)f.out)[i] = (u8)v; break;
                            default: ((u64*)f.out)[i] = v; break;
                        }
                        if (f.out_nulls) f.out_nulls[i] = rows > 0 ? (u8)0 : (u8)1;
                    }
                    break;
                }
                case PA_WINDOW_LAG:
                case PA_WINDOW_LEAD:
                case PA_WINDOW_FIRST_VALUE:
                case PA_WINDOW_LAST_VALUE:
                case PA_WINDOW_NTH_VALUE: {
                    // the place the value is copied from, inside [0, N); lag / lead outside it: the default at the current row
                    const bool shifted = f.function == PA_WINDOW_LAG || f.function == PA_WINDOW_LEAD;
                    const i64 e = f.frame_end == kWindowFrameRow ? place : f.frame_end == kWindowFramePeers ? pe - 1 : N - 1;
                    i64 row = 0;   // the current row as held: where the offset and the default are read
                    if (f.offset_values || f.default_values) {
                        row = a.perm[i];
                        row = row < 0 ? 0 : row > (i64)n - 1 ? (i64)n - 1 : row;
                    }
                    i64 offset = 1;
                    bool is_null = false, use_default = false;
                    if (f.offset_values) {
                        is_null = f.offset_nulls && f.offset_nulls[row];
                        offset = f.offset_type == PA_BIGINT ? ((const i64*)f.offset_values)[row] : (i64)((const i32*)f.offset_values)[row];
                    }
                    i64 target = 0;
                    if (f.function == PA_WINDOW_LAST_VALUE) target = e;
                    else if (shifted && !is_null) {
                        // (offset against the rows in front of / behind the place: place - offset, place + offset could leave int64)
                        const i64 room = f.function == PA_WINDOW_LAG ? place : N - 1 - place;
                        if (offset < 0) {
                            atomicOr(a.error, kWindowErrorLagOffset);
                            is_null = true;
                        }
                        else if (offset > room) use_default = true;
                        else target = f.function == PA_WINDOW_LAG ? place - offset : place + offset;
                    }
                    else if (f.function == PA_WINDOW_NTH_VALUE && !is_null) {
                        if (offset < 1) {
                            atomicOr(a.error, kWindowErrorNthOffset);
                            is_null = true;
                        }
                        else if (offset - 1 > e) is_null = true;
                        else target = offset - 1;
                    }
                    const void* values = f.arg_values;
                    const u8* nulls = f.arg_nulls;
                    i64 src = row;
                    if (use_default) {
                        values = f.default_values;
                        nulls = f.default_nulls;
                        if (!values) is_null = true;
                    }
                    else if (!is_null) {
                        i64 at = first + target;
                        at = at < 0 ? 0 : at > (i64)n - 1 ? (i64)n - 1 : at;
                        src = a.perm[at];
                        src = src < 0 ? 0 : src > (i64)n - 1 ? (i64)n - 1 : src;
                    }
                    if (!is_null && nulls && nulls[src]) is_null = true;
                    // the very bytes of the source row at the type's width; a NULL result holds zeros
                    switch (f.width) {
                        case 1: ((u8*)f.out)[i] = is_null ? (u8)0 : ((const u8*)values)[src]; break;
                        case 4: ((u32*)f.out)[i] = is_null ? 0u : ((const u32*)values)[src]; break;
                        case 8: ((u64*)f.out)[i] = is_null ? 0ULL : ((const u64*)values)[src]; break;
                        default: {
                            const u64 lo = is_null ? 0ULL : ((const u64*)values)[2 * src], hi = is_null ? 0ULL : ((const u64*)values)[2 * src + 1];
                            ((u64*)f.out)[2 * i] = lo;
                            ((u64*)f.out)[2 * i + 1] = hi;
                            break;
                        }
                    }
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

void launch_window_gather(int32_t type, const void* values, const uint8_t* nulls, const int32_t* perm, int32_t n, uint64_t* sorted_values,
                          uint8_t* sorted_nulls, hipStream_t s)
{
    if (n <= 0 || (sorted_values == nullptr && sorted_nulls == nullptr)) return;
    hipLaunchKernelGGL(k_window_gather, grid_of(n), 256, 0, s, type, values, nulls, perm, n, (u64*)sorted_values, sorted_nulls);
    PA_HIP(hipGetLastError());
}

namespace {
inline int64_t scan_tiles(int32_t n) { return ((int64_t)n + kWindowScanTile - 1) / kWindowScanTile; }

template <int KIND>
void launch_window_scan_of(int mode, const u64* values, const uint8_t* nulls, const int32_t* part_flag, int32_t n, void* out, int32_t* error, void* temp, hipStream_t s)
{
    const int tiles = (int)scan_tiles(n);
    WindowAcc* tile_acc = static_cast<WindowAcc*>(temp);
    WindowAcc* tile_front = tile_acc + tiles;
    hipLaunchKernelGGL(k_window_scan_tiles<KIND>, tiles, 256, 0, s, values, nulls, part_flag, n, mode, tile_acc);
    hipLaunchKernelGGL(k_window_scan_tile_fronts<KIND>, 1, 256, 0, s, (const WindowAcc*)tile_acc, (i32)tiles, mode, tile_front);
    hipLaunchKernelGGL(k_window_scan_apply<KIND>, tiles, 256, 0, s, values, nulls, part_flag, n, mode, (const WindowAcc*)tile_front, out, error);
    PA_HIP(hipGetLastError());
}
}  // namespace

size_t window_scan_temp_bytes(int32_t n) { return (size_t)(2 * scan_tiles(n) + 1) * sizeof(WindowAcc); }

void launch_window_scan(WindowScanKind kind, bool floating, const uint64_t* sorted_values, const uint8_t* sorted_nulls, const int32_t* part_flag,
                        int32_t n, void* out, int32_t* error, void* temp, hipStream_t s)
{
    if (n <= 0) return;
    const u64* v = (const u64*)sorted_values;
    switch (kind) {
        case kWindowScanCount: launch_window_scan_of<kWindowScanCount>(kCmpInt, v, sorted_nulls, part_flag, n, out, error, temp, s); break;
        case kWindowScanSum: launch_window_scan_of<kWindowScanSum>(kCmpInt, v, sorted_nulls, part_flag, n, out, error, temp, s); break;
        case kWindowScanMin: launch_window_scan_of<kWindowScanMin>(floating ? kCmpDoubleMin : kCmpInt, v, sorted_nulls, part_flag, n, out, error, temp, s); break;
        case kWindowScanMax: launch_window_scan_of<kWindowScanMax>(floating ? kCmpDoubleMax : kCmpInt, v, sorted_nulls, part_flag, n, out, error, temp, s); break;
    }
}

void launch_window_functions(const WindowFunctionArgs& a, hipStream_t s)
{
    if (a.n <= 0 || a.count <= 0) return;
    const int blocks = (int)(((int64_t)a.n + kWindowRowsPerBlock - 1) / kWindowRowsPerBlock);
    hipLaunchKernelGGL(k_window_functions, blocks, 256, 0, s, a);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
