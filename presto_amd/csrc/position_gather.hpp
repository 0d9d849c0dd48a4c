// position_gather.hpp -- PositionGather: Block.copyPositions of one channel on the device, the one copy of it for every operator.
//
//   copy_varwidth     VariableWidthBlock.copyPositions without the NULL flags: lengths through the position list -> exclusive scan ->
//                     the byte total to the host (ONE read-back) -> the byte buffer sized from it -> the bytes and offsets[k]
//   copy_positions    a whole channel into an OutColumn: NULL flags, then fixed-width values or copy_varwidth
// positions may be null (identity) and may hold -1 (a NULL row: length 0).  A VARCHAR channel costs one read-back (one stream
// synchronisation) per call, a fixed-width channel none.
// The 2 GiB limit: the scan adds the lengths in 32 bits, so its total alone says nothing about a column of 2 GiB and more.
// checked_varwidth_offsets is the one place that turns lengths into offsets AND a total a buffer may be sized by: it adds the lengths in
// 64 bits as well and refuses 2^31 bytes and more before anything is sized or written.  copy_varwidth goes through it when the caller
// passes over_2gib_message (the joins: their output rows multiply); so do the page stager's dictionary / RLE decode, the interner's
// decode and the ABI helpers.  A caller of copy_varwidth / copy_positions WITHOUT a message gathers a subset or a permutation of the rows
// of ONE staged block or held column, which holds under 2 GiB (PageStager::stage and HeldRows::append_offsets refuse more), so its total
// does too: each such call site says which block that is.
#pragma once

#include "device_page.hpp"
#include "join_kernels.hpp"
#include "scan_kernels.hpp"

namespace pa {

// lengths in offs[0..n) -> offsets from 0 in offs[0..n) (exclusive scan in place; the caller, or launch_varwidth_copy through total_dev,
// writes offs[n]).  Returns the byte total added in 64 bits, and throws PA_ERR_INSUFFICIENT_RESOURCES with over_2gib_message when it
// is 2^31 or more: BEFORE the caller sizes the byte buffer or launches the copy.  total_dev: 16 bytes of device scratch
// [the scan's 32-bit total, -, the 64-bit sum]; scan_temp: scan_temp_bytes(n).  One read-back (one stream synchronisation).
// true_total (may be null) receives the 64-bit total also when it is refused.
inline int64_t checked_varwidth_offsets(int32_t* offs, int64_t n, int32_t* total_dev, void* scan_temp, hipStream_t s, const char* over_2gib_message,
                                        int64_t* true_total = nullptr)
{
    launch_sum_i32_i64(offs, n, reinterpret_cast<int64_t*>(total_dev + 2), s);
    launch_exclusive_scan_i32(offs, offs, n, total_dev, scan_temp, s);
    int32_t h_total[4] = {0, 0, 0, 0};
    read_back(h_total, total_dev, 16, s);
    int64_t bytes64;
    memcpy(&bytes64, h_total + 2, 8);
    if (true_total) *true_total = bytes64;
    PA_REQUIRE(bytes64 >= 0 && bytes64 < ((int64_t)1 << 31), PA_ERR_INSUFFICIENT_RESOURCES, over_2gib_message);
    return bytes64;
}

class PositionGather {
public:
    // k + 1 offsets from 0 into offsets_buf, the bytes into values_buf (both grown here); returns the byte total
    int32_t copy_varwidth(const DevColumn& src, const int32_t* positions, int32_t k, DevBuf& offsets_buf, DevBuf& values_buf, hipStream_t s,
                          const char* over_2gib_message = nullptr)
    {
        int32_t* offs = static_cast<int32_t*>(offsets_buf.ensure((size_t)(k + 1) * 4));
        int32_t* total = static_cast<int32_t*>(total_.ensure(64));   // [the scan's total, -, the 64-bit sum of the lengths]
        launch_varwidth_lengths(positions, k, src.offsets, src.nulls, offs, s);
        int32_t h_total = 0;
        if (over_2gib_message) h_total = (int32_t)checked_varwidth_offsets(offs, k, total, scan_temp_.ensure(scan_temp_bytes(k)), s, over_2gib_message);
        else {
            // (the caller's rows come out of one block under 2 GiB: see the head of this file)
            launch_exclusive_scan_i32(offs, offs, k, total, scan_temp_.ensure(scan_temp_bytes(k)), s);
            read_back(&h_total, total, 4, s);
        }
        uint8_t* bytes = static_cast<uint8_t*>(values_buf.ensure((size_t)(h_total > 0 ? h_total : 1)));
        launch_varwidth_copy(positions, k, src.offsets, static_cast<const uint8_t*>(src.values), src.nulls, offs, bytes, total, s);
        return h_total;
    }

    // Block.copyPositions of one channel; returns the VARCHAR byte total (0 for a fixed-width channel)
    int32_t copy_positions(const DevColumn& src, const int32_t* positions, int32_t k, OutColumn& o, hipStream_t s)
    {
        o.type = src.type;
        o.varwidth = src.varwidth;
        o.has_nulls = src.nulls != nullptr;
        o.is_view = false;
        o.host_ready = false;
        if (src.nulls) launch_gather_nulls(src.nulls, positions, k, static_cast<uint8_t*>(o.nulls.ensure((size_t)k)), s);
        if (src.varwidth) return copy_varwidth(src, positions, k, o.offsets, o.values, s);
        const int w = type_width(src.type);
        launch_gather_flat(src.values, w, positions, k, o.values.ensure((size_t)k * w), s);
        return 0;
    }

    size_t bytes() const { return scan_temp_.capacity() + total_.capacity(); }

private:
    DevBuf scan_temp_, total_;
};

}  // namespace pa
