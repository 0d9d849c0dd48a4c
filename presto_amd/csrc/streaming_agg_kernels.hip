// streaming_agg_kernels.hip -- the passes of StreamingAggregationOperator (streaming_agg_kernels.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "streaming_agg_kernels.hpp"
#include "kernels/pa_row_distinct.h"

namespace pa {

namespace {

// ---- flags ---------------------------------------------------------------------------------------------------------------------------
// pa_row_distinct.h's IS DISTINCT FROM between row a of one column and row b of another of the same type (the page and the carry)
__device__ __forceinline__ bool key_distinct(i32 type, const void* __restrict__ va, const i32* __restrict__ oa, const u8* __restrict__ na, i64 a,
                                             const void* __restrict__ vb, const i32* __restrict__ ob, const u8* __restrict__ nb, i64 b)
{
    const bool xa = na && na[a], xb = nb && nb[b];
    if (xa || xb) return xa != xb;
    switch (type) {
        case PA_BIGINT:
        case PA_DECIMAL: return ((const i64*)va)[a] != ((const i64*)vb)[b];
        case PA_INTEGER:
        case PA_DATE: return ((const i32*)va)[a] != ((const i32*)vb)[b];
        case PA_BOOLEAN: return (((const u8*)va)[a] != 0) != (((const u8*)vb)[b] != 0);
        case PA_DOUBLE: return float_distinct<true>(((const double*)va)[a], ((const double*)vb)[b]);
        case PA_REAL: return float_distinct<true>(((const float*)va)[a], ((const float*)vb)[b]);
        case PA_VARCHAR: {
            const i32 sa = oa[a], sb = ob[b], la = oa[a + 1] - sa, lb = ob[b + 1] - sb;
            if (la != lb) return true;
            const u8* pa_ = (const u8*)va + sa;
            const u8* pb_ = (const u8*)vb + sb;
            for (i32 j = 0; j < la; j++)
                if (pa_[j] != pb_[j]) return true;
            return false;
        }
        default: return true;
    }
}

// one flag per row over all group channels, in page order; the channel loop is unrolled so that the channels are read out of the kernel
// arguments by constant index
__global__ __launch_bounds__(256) void k_stream_agg_flags(StreamAggFlagArgs a)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (i64)gridDim.x * 256) {
        bool differs = false;
#pragma unroll
        for (int c = 0; c < kStreamAggMaxKeys; c++) {
            if (c >= a.count || differs) continue;
            const StreamAggKey& k = a.k[c];
            if (i > 0) differs = row_distinct<true>(k.type, k.values, k.offsets, k.nulls, i - 1, i);
            else if (a.open) differs = key_distinct(k.type, k.carry_values, k.carry_offsets, k.carry_nulls, 0, k.values, k.offsets, k.nulls, 0);
        }
        a.flags[i] = differs ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_stream_agg_starts(const i32* __restrict__ flags, const i32* __restrict__ idx, i32 n, i32* __restrict__ start)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const i32 f = flags[i];
        if (f) start[idx[i] + 1] = (i32)i;   // idx[i] + 1 in [1, i + 1]: one writer, the run's first row
        if (i == 0) start[0] = 0;            // run 0: row 0 when nothing is carried in, else the carried run's placeholder
    }
}

// ---- the segmented reduction ---------------------------------------------------------------------------------------------------------------
typedef StreamAggState Acc;
constexpr i32 kRestart = 1, kHas = 2;

__device__ __forceinline__ double acc_double(const Acc& x) { return __longlong_as_double((long long)x.a); }
__device__ __forceinline__ u64 acc_count(const Acc& x) { return ((u64)(u32)(x.f >> 1) << 32) | (u64)(u32)x.b; }

// the key under which min / max compare: smaller key = smaller value (agg_model.compare)
__device__ __forceinline__ i64 minmax_key(u64 bits, int cmp)
{
    if (cmp == kStreamAggCmpInt) return (i64)bits;
    const double d = cmp == kStreamAggCmpFloat ? (double)__int_as_float((int)(u32)bits) : __longlong_as_double((long long)bits);
    if (d != d) return 0x7FFFFFFFFFFFFFFFLL;                      // every NaN one value, above +infinity
    const i64 b = (i64)__double_as_longlong(d);
    return b < 0 ? (b ^ 0x7FFFFFFFFFFFFFFFLL) : b;                // Double.compare order: -0.0 -> -1, +0.0 -> 0
}

// x before y: where y holds a run start, what came before it is dropped.  (Selects field by field, no early return: a choice between two
// structs would leave them in scratch.)
__device__ __forceinline__ Acc acc_combine(const Acc& x, const Acc& y, int kind, int cmp)
{
    const bool restart = (y.f & kRestart) != 0;
    Acc r;
    if (kind == kStreamAggCount) {
        r.a = restart ? y.a : x.a + y.a;
        r.b = 0;
        r.f = (x.f | y.f) & kRestart;
    }
    else if (kind == kStreamAggSumInt) {
        const u64 lo = x.a + y.a;
        r.a = restart ? y.a : lo;
        r.b = restart ? y.b : x.b + y.b + (lo < x.a ? 1 : 0);
        r.f = ((x.f | y.f) & kRestart) | (restart ? (y.f & kHas) : ((x.f | y.f) & kHas));
    }
    else if (kind == kStreamAggSumDouble) {
        const double sum = acc_double(x) + acc_double(y);
        r.a = restart ? y.a : (u64)__double_as_longlong(sum);
        const u64 count = restart ? acc_count(y) : acc_count(x) + acc_count(y);
        r.b = (i32)(u32)count;
        r.f = ((x.f | y.f) & kRestart) | (i32)((u32)(count >> 32) << 1);
    }
    else {
        const i64 kx = minmax_key(x.a, cmp), ky = minmax_key(y.a, cmp);
        const bool better = kind == kStreamAggMin ? ky < kx : ky > kx;
        // keep the left unless there is none or the right is strictly better
        const bool take = restart || !(x.f & kHas) || ((y.f & kHas) && better);
        r.a = take ? y.a : x.a;
        r.b = 0;
        r.f = ((x.f | y.f) & kRestart) | ((take ? y.f : x.f) & kHas);
    }
    return r;
}
__device__ __forceinline__ Acc acc_shfl_up(const Acc& v, int off)
{
    Acc o;
    o.a = (u64)__shfl_up((long long)v.a, off, 64);
    o.b = __shfl_up(v.b, off, 64);
    o.f = __shfl_up(v.f, off, 64);
    return o;
}
__device__ __forceinline__ Acc acc_identity()
{
    Acc r;
    r.a = 0;   // count 0, sum 0, +0.0
    r.b = 0;
    r.f = 0;
    return r;
}

// The four consecutive entries of a lane, combined in place (s[j] = e[0] + ... + e[j]), then over the 256 lanes of the workgroup: the
// state of everything in front of the lane's entries inside the workgroup (returned) and of the whole workgroup (*total).
__device__ __forceinline__ Acc acc_block_scan(Acc (&s)[4], int kind, int cmp, Acc* total)
{
    __shared__ Acc wave_total[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 1; j < 4; j++) s[j] = acc_combine(s[j - 1], s[j], kind, cmp);
    Acc inc = s[3];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const Acc o = acc_shfl_up(inc, off);
        if (lane >= off) inc = acc_combine(o, inc, kind, cmp);
    }
    if (lane == 63) wave_total[wave] = inc;
    Acc before = acc_shfl_up(inc, 1);
    if (lane == 0) before = acc_identity();
    __syncthreads();
    Acc front = acc_identity(), all = acc_identity();
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const Acc t = wave_total[w];
        if (w < wave) front = acc_combine(front, t, kind, cmp);
        all = acc_combine(all, t, kind, cmp);
    }
    __syncthreads();
    *total = all;
    return acc_combine(front, before, kind, cmp);
}

// the entry of row i: what the row adds to its run, with the run-start flag
__device__ __forceinline__ Acc acc_of_row(const StreamAggFn& f, i64 i, i32 flag)
{
    Acc e = acc_identity();
    e.f = flag ? kRestart : 0;
    bool counted = true;
    if (f.mask_values) counted = !(f.mask_nulls && f.mask_nulls[i]) && f.mask_values[i] != 0;   // a NULL mask is false
    if (f.fn != PA_AGG_COUNT_STAR && f.nulls && f.nulls[i]) counted = false;
    if (!counted) return e;
    if (f.kind == kStreamAggCount) {
        e.a = 1;
        return e;
    }
    if (f.kind == kStreamAggSumInt) {
        const i64 v = f.in_type == PA_BIGINT ? ((const i64*)f.values)[i] : (i64)((const i32*)f.values)[i];
        e.a = (u64)v;
        e.b = v < 0 ? -1 : 0;
        e.f |= kHas;
        return e;
    }
    if (f.kind == kStreamAggSumDouble) {
        double d;
        switch (f.in_type) {
            case PA_BIGINT: d = (double)((const i64*)f.values)[i]; break;
            case PA_INTEGER: d = (double)((const i32*)f.values)[i]; break;
            case PA_REAL: d = (double)((const float*)f.values)[i]; break;
            default: d = ((const double*)f.values)[i]; break;
        }
        e.a = (u64)__double_as_longlong(d);
        e.b = 1;
        return e;
    }
    switch (f.in_type) {   // min / max: the value's own bits
        case PA_INTEGER:
        case PA_DATE: e.a = (u64)(i64)((const i32*)f.values)[i]; break;
        case PA_REAL: e.a = (u64)((const u32*)f.values)[i]; break;
        case PA_BOOLEAN: e.a = ((const u8*)f.values)[i] ? 1ULL : 0ULL; break;
        default: e.a = ((const u64*)f.values)[i]; break;   // BIGINT, short DECIMAL, DOUBLE
    }
    e.f |= kHas;
    return e;
}

__device__ __forceinline__ bool sum_leaves_int64(const Acc& r) { return r.b != ((i64)r.a < 0 ? -1 : 0); }

// the finished value of a run into row `run` of the aggregate's output column; false: the run has no result (kStreamAggErrorClosed)
__device__ __forceinline__ bool acc_store(const StreamAggFn& f, const Acc& r, i64 run)
{
    if (f.kind == kStreamAggCount) {
        ((i64*)f.out)[run] = (i64)r.a;
        return true;
    }
    bool ok = true;
    if (f.kind == kStreamAggSumInt) {
        const bool has = (r.f & kHas) != 0;
        f.out_nulls[run] = has ? 0 : 1;
        if (f.in_type == PA_BIGINT) {
            ok = !sum_leaves_int64(r);
            ((i64*)f.out)[run] = (i64)r.a;
        }
        else {   // the INTEGER result column: the int64 total, then the column's range
            const i64 v = (i64)r.a;
            ok = !sum_leaves_int64(r) && v >= -2147483648LL && v <= 2147483647LL;
            ((i32*)f.out)[run] = (i32)v;
        }
        return ok || !has;
    }
    if (f.kind == kStreamAggSumDouble) {
        const u64 count = acc_count(r);
        f.out_nulls[run] = count ? 0 : 1;
        const double sum = 0.0 + acc_double(r);   // the reference's state starts at +0.0: a run of -0.0 alone sums to +0.0
        const double v = f.fn == PA_AGG_AVG ? sum / (double)count : sum;
        if (f.in_type == PA_REAL) ((float*)f.out)[run] = count ? (float)v : 0.0f;
        else ((double*)f.out)[run] = count ? v : 0.0;
        return true;
    }
    const bool has = (r.f & kHas) != 0;
    f.out_nulls[run] = has ? 0 : 1;
    switch (f.in_type) {
        case PA_INTEGER:
        case PA_DATE:
        case PA_REAL: ((u32*)f.out)[run] = has ? (u32)r.a : 0u; break;
        case PA_BOOLEAN: ((u8*)f.out)[run] = has ? (u8)r.a : (u8)0; break;
        default: ((u64*)f.out)[run] = has ? r.a : 0ULL; break;
    }
    return true;
}

__device__ __forceinline__ void acc_load_rows(Acc (&s)[4], i32 (&flag)[4], const StreamAggFn& f, i64 base, i32 n, const i32* __restrict__ flags)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const i64 i = base + j;
        flag[j] = 0;
        s[j] = acc_identity();
        if (i >= n) continue;
        flag[j] = flags[i];
        s[j] = acc_of_row(f, i, flag[j]);
    }
}

// launch 1 of 3: the state of every tile of kStreamAggTile rows; blockIdx.y = the aggregate
__global__ __launch_bounds__(256) void k_stream_agg_tiles(StreamAggArgs a)
{
    const StreamAggFn f = a.f[blockIdx.y];
    Acc s[4], total;
    i32 flag[4];
    acc_load_rows(s, flag, f, (i64)blockIdx.x * kStreamAggTile + (i64)threadIdx.x * 4, a.n, a.flags);
    (void)acc_block_scan(s, f.kind, f.cmp, &total);
    if (threadIdx.x == 0) a.tile_acc[(i64)blockIdx.y * a.tiles + blockIdx.x] = total;
}

// launch 2 of 3, one workgroup per aggregate: tile_front[t] = the carried state and the tiles in front of tile t, kStreamAggTile tiles at a time
__global__ __launch_bounds__(256) void k_stream_agg_tile_fronts(StreamAggArgs a)
{
    const StreamAggFn f = a.f[blockIdx.y];
    const Acc* __restrict__ tile_acc = a.tile_acc + (i64)blockIdx.y * a.tiles;
    Acc* __restrict__ tile_front = a.tile_front + (i64)blockIdx.y * a.tiles;
    Acc carry = acc_identity();
    if (a.open) {   // the open run's state seeds the page; a flag on row 0 drops it again
        carry = a.carry_in[blockIdx.y];
        carry.f &= ~kRestart;
    }
    for (i32 chunk = 0; chunk < a.tiles; chunk += kStreamAggTile) {
        const i32 base = chunk + (i32)threadIdx.x * 4;
        Acc e[4], s[4], total;
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = e[j] = base + j < a.tiles ? tile_acc[base + j] : acc_identity();
        Acc front = acc_combine(carry, acc_block_scan(s, f.kind, f.cmp, &total), f.kind, f.cmp);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (base + j < a.tiles) tile_front[base + j] = front;
            front = acc_combine(front, e[j], f.kind, f.cmp);
        }
        carry = acc_combine(carry, total, f.kind, f.cmp);
    }
}

// launch 3 of 3: the tile's own scan behind the state in front of it, kept in registers; stored are the values of the runs that end in
// the tile, and the state at row n - 1
__global__ __launch_bounds__(256) void k_stream_agg_apply(StreamAggArgs a)
{
    const StreamAggFn f = a.f[blockIdx.y];
    const i64 base = (i64)blockIdx.x * kStreamAggTile + (i64)threadIdx.x * 4;
    Acc s[4], total;
    i32 flag[4];
    acc_load_rows(s, flag, f, base, a.n, a.flags);
    const Acc front = acc_combine(a.tile_front[(i64)blockIdx.y * a.tiles + blockIdx.x], acc_block_scan(s, f.kind, f.cmp, &total), f.kind, f.cmp);
    const bool exact_sum = f.kind == kStreamAggSumInt && f.in_type == PA_BIGINT;
    const i32 closed = *a.closed;
    i32 error = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const i64 i = base + j;
        if (i >= a.n) continue;
        const Acc r = acc_combine(front, s[j], f.kind, f.cmp);
        const i32 run = a.idx[i] + flag[j];
        // Math.addExact in row order: every prefix of the run's counted values (a row that is not counted repeats the prefix before it)
        if (exact_sum && sum_leaves_int64(r)) error |= run < closed ? kStreamAggErrorClosed : kStreamAggErrorOpen;
        if (i + 1 < a.n && a.flags[i + 1]) {
            if (!acc_store(f, r, run)) error |= kStreamAggErrorClosed;
        }
        if (i == a.n - 1) {
            Acc last = r;
            last.f &= ~kRestart;
            a.carry_out[blockIdx.y] = last;
        }
        if (i == 0 && flag[j]) {   // (only with a run carried in) that run ended with the page before: its state is its result
            if (!acc_store(f, a.carry_in[blockIdx.y], 0)) error |= kStreamAggErrorClosed;
        }
    }
    if (error) atomicOr(a.error, error);
}

// the open run's row at finish: one workgroup of one lane per aggregate
__global__ void k_stream_agg_finish(StreamAggArgs a)
{
    const StreamAggFn f = a.f[blockIdx.x];
    if (threadIdx.x != 0) return;
    if (!acc_store(f, a.carry_in[blockIdx.x], 0)) atomicOr(a.error, kStreamAggErrorClosed);
}

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)device_cu_count() * 8)); }

}  // namespace

void launch_stream_agg_flags(const StreamAggFlagArgs& a, hipStream_t s)
{
    PA_REQUIRE(a.n > 0 && a.count >= 1 && a.count <= kStreamAggMaxKeys && a.flags != nullptr, PA_ERR_DEVICE, "streaming aggregation: bad flag arguments");
    hipLaunchKernelGGL(k_stream_agg_flags, grid_for(a.n), 256, 0, s, a);
    PA_HIP(hipGetLastError());
}

void launch_stream_agg_starts(const int32_t* flags, const int32_t* idx, int32_t n, int32_t* start, hipStream_t s)
{
    hipLaunchKernelGGL(k_stream_agg_starts, grid_for(n), 256, 0, s, flags, idx, n, start);
    PA_HIP(hipGetLastError());
}

void launch_stream_agg_reduce(const StreamAggArgs& a, hipStream_t s)
{
    PA_REQUIRE(a.n > 0 && a.count >= 1 && a.count <= kStreamAggMaxAggregates && a.tiles == stream_agg_tiles(a.n), PA_ERR_DEVICE,
               "streaming aggregation: bad reduce arguments");
    const dim3 tiles((unsigned)a.tiles, (unsigned)a.count);
    hipLaunchKernelGGL(k_stream_agg_tiles, tiles, 256, 0, s, a);
    hipLaunchKernelGGL(k_stream_agg_tile_fronts, dim3(1, (unsigned)a.count), 256, 0, s, a);
    hipLaunchKernelGGL(k_stream_agg_apply, tiles, 256, 0, s, a);
    PA_HIP(hipGetLastError());
}

void launch_stream_agg_finish(const StreamAggArgs& a, hipStream_t s)
{
    PA_REQUIRE(a.count >= 1 && a.count <= kStreamAggMaxAggregates, PA_ERR_DEVICE, "streaming aggregation: bad finish arguments");
    hipLaunchKernelGGL(k_stream_agg_finish, (unsigned)a.count, 64, 0, s, a);
    PA_HIP(hipGetLastError());
}

}  // namespace pa
