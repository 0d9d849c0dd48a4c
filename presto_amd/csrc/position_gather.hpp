// position_gather.hpp -- PositionGather: Block.copyPositions of one channel on the device, the one copy of it for every operator.
//
//   copy_varwidth     VariableWidthBlock.copyPositions without the NULL flags: lengths through the position list -> exclusive scan ->
//                     the byte total to the host (ONE read-back) -> the byte buffer sized from it -> the bytes and offsets[k]
//   copy_positions    a whole channel into an OutColumn: NULL flags, then fixed-width values or copy_varwidth
// positions may be null (identity) and may hold -1 (a NULL row: length 0).  A VARCHAR channel costs one read-back (one stream
// synchronisation) per call, a fixed-width channel none.
// The 2 GiB limit: the scan adds the lengths in 32 bits.  Only a caller that passes over_2gib_message has the total checked in 64 bits
// (the join: its output rows multiply).  Every other caller gathers rows out of ONE block or held column, and relies on its own
// caller's guarantee that such a block holds under 2 GiB of bytes, so a subset of its rows does too.
#pragma once

#include "device_page.hpp"
#include "join_kernels.hpp"
#include "scan_kernels.hpp"

namespace pa {

class PositionGather {
public:
    // k + 1 offsets from 0 into offsets_buf, the bytes into values_buf (both grown here); returns the byte total
    int32_t copy_varwidth(const DevColumn& src, const int32_t* positions, int32_t k, DevBuf& offsets_buf, DevBuf& values_buf, hipStream_t s,
                          const char* over_2gib_message = nullptr)
    {
        int32_t* offs = static_cast<int32_t*>(offsets_buf.ensure((size_t)(k + 1) * 4));
        int32_t* total = static_cast<int32_t*>(total_.ensure(64));   // [the scan's total, -, the 64-bit sum of the lengths]
        launch_varwidth_lengths(positions, k, src.offsets, src.nulls, offs, s);
        if (over_2gib_message) launch_sum_i32_i64(offs, k, reinterpret_cast<int64_t*>(total + 2), s);
        launch_exclusive_scan_i32(offs, offs, k, total, scan_temp_.ensure(scan_temp_bytes(k)), s);
        int32_t h_total[4] = {0, 0, 0, 0};
        read_back(h_total, total, over_2gib_message ? 16 : 4, s);
        if (over_2gib_message) {
            int64_t bytes64;
            memcpy(&bytes64, h_total + 2, 8);
            PA_REQUIRE(bytes64 < ((int64_t)1 << 31), PA_ERR_INSUFFICIENT_RESOURCES, over_2gib_message);
        }
        uint8_t* bytes = static_cast<uint8_t*>(values_buf.ensure((size_t)(h_total[0] > 0 ? h_total[0] : 1)));
        launch_varwidth_copy(positions, k, src.offsets, static_cast<const uint8_t*>(src.values), src.nulls, offs, bytes, total, s);
        return h_total[0];
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
