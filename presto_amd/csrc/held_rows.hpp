// held_rows.hpp -- HeldRows: rows collected page by page, column by column on the device (the reference's PagesIndex: flat arrays,
// address == position).  One append for every operator that accumulates rows:
//   OrderBy (op_order_by.cpp), Window (op_window.cpp), TopNRanking (op_topn_ranking.cpp)   their input, sorted through a permutation
//   HashBuilder (op_join.cpp)               the build rows of a lookup source (LookupSourceImpl::rows, join_source.hpp)
//   LookupJoin, NestedLoopJoin              a probe page that comes out over several calls and must outlive its producer's next one
//   FilterAndProject (op_filter_project.cpp) the MergePages buffer
//
//   append_page / append_positions    PagesIndex.addPage: a staged page (or its rows at `positions`) behind the rows held
//   append_column                     one column of a page whose VARCHAR ends the caller knows already (the caller counts the rows)
//   keep_positions                    the rows at `rowids` into fresh columns (a prune)
//   gather_sorted                     PagesIndex.appendTo: channels through a permutation into output columns
//   reset                             no rows held, the allocations kept
// The rules that live here and nowhere else: the first page with NULLs allocates a column's flags and clears the rows held before it;
// VARCHAR offsets are rebased onto the bytes used; a VARCHAR column of more than INT32_MAX bytes is refused.
// Host cost per VARCHAR channel and call: one read-back of 4 bytes (append_page: two 4-byte copies), one stream sync; a fixed-width
// channel costs none.  The gathers by position are PositionGather's (position_gather.hpp).  Nothing here waits at the end of a call: the callers keep their own.  The row-count limit of a
// sort stays with the operators (they word it differently, and TopNRanking prunes before it gives up).
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "device_page.hpp"
#include "position_gather.hpp"
#include "scan_kernels.hpp"
#include "static_kernels.hpp"

// (internal to the library: the inline functions here stay out of its exported symbols)
#pragma GCC visibility push(hidden)

namespace pa {

struct HeldRows {
    // held: the channels kept (every other column stays empty)
    void init(const std::vector<int32_t>& types, const std::vector<bool>& held_mask)
    {
        held = held_mask;
        cols.resize(types.size());
        var_bytes.assign(types.size(), 0);
        for (size_t c = 0; c < types.size(); c++) {
            cols[c].type = types[c];
            cols[c].varwidth = types[c] == PA_VARCHAR;
        }
    }

    // the m rows of a staged page behind the rows held
    void append_page(const DevPage& in, int64_t m, hipStream_t s)
    {
        for (size_t c = 0; c < cols.size(); c++) {
            if (!held[c]) continue;
            const DevColumn& src = in.cols[c];
            PA_REQUIRE(src.type == cols[c].type, PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared input type");
            int32_t ends[2] = {0, 0};
            if (cols[c].varwidth) read_offset_ends(src.offsets, m, ends, s);
            append_column(c, src, m, ends[0], (int64_t)ends[1] - ends[0], s);
        }
        rows += m;
    }

    // the m rows of one column behind the rows held; a VARCHAR's bytes are [first, first + add) of src.values.  `rows` is the caller's
    // to advance, once every column of the page is in.
    void append_column(size_t c, const DevColumn& src, int64_t m, int32_t first, int64_t add, hipStream_t s)
    {
        OutColumn& h = cols[c];
        if (h.varwidth) {
            char* v = append_offsets(c, src.offsets, m, add, s);
            if (add) PA_HIP(hipMemcpyAsync(v, static_cast<const char*>(src.values) + first, (size_t)add, hipMemcpyDeviceToDevice, s));
        }
        else {
            const size_t w = (size_t)type_width(h.type);
            char* v = static_cast<char*>(h.values.reserve_keep((size_t)room(m) * w, (size_t)rows * w, s));
            PA_HIP(hipMemcpyAsync(v + (size_t)rows * w, src.values, (size_t)m * w, hipMemcpyDeviceToDevice, s));
        }
        if (uint8_t* nl = append_nulls(h, src.nulls != nullptr, m, s)) PA_HIP(hipMemcpyAsync(nl, src.nulls, (size_t)m, hipMemcpyDeviceToDevice, s));
    }

    // no rows held; the allocations stay
    void reset()
    {
        rows = 0;
        std::fill(var_bytes.begin(), var_bytes.end(), 0);
        for (OutColumn& o : cols) o.has_nulls = false;
    }

    // Block.copyPositions: the k rows of a staged page at `positions` behind the rows held (varchar_tmp: the caller's scratch column)
    void append_positions(const DevPage& in, const int32_t* positions, int32_t k, PositionGather& gather, OutColumn& varchar_tmp, hipStream_t s)
    {
        for (size_t c = 0; c < cols.size(); c++) {
            if (!held[c]) continue;
            const DevColumn& src = in.cols[c];
            OutColumn& h = cols[c];
            if (h.varwidth) {
                // (no 2 GiB message: a subset of the rows of ONE staged block, which holds under 2 GiB -- PageStager::stage; the sum with the rows held is checked in append_offsets)
                const int32_t add = gather.copy_positions(src, positions, k, varchar_tmp, s);   // offsets from 0, k + 1 of them
                char* v = append_offsets(c, varchar_tmp.offsets.as<int32_t>(), k, add, s);
                if (add) PA_HIP(hipMemcpyAsync(v, varchar_tmp.values.ptr(), (size_t)add, hipMemcpyDeviceToDevice, s));
            }
            else {
                const size_t w = (size_t)type_width(h.type);
                char* v = static_cast<char*>(h.values.reserve_keep((size_t)room(k) * w, (size_t)rows * w, s));
                launch_gather_flat(src.values, (int)w, positions, k, v + (size_t)rows * w, s);
            }
            if (uint8_t* nl = append_nulls(h, src.nulls != nullptr, k, s)) launch_gather_nulls(src.nulls, positions, k, nl, s);
        }
        rows += k;
    }

    // the rows at `rowids` (positions among the rows held) into fresh columns, in that order; they are the rows held afterwards
    void keep_positions(const int32_t* rowids, int32_t kept, PositionGather& gather, hipStream_t s)
    {
        for (size_t c = 0; c < cols.size(); c++) {
            if (!held[c]) continue;
            OutColumn fresh;
            // (no 2 GiB message: the callers keep each held row at most once, and the held column is at most INT32_MAX bytes -- append_offsets)
            var_bytes[c] = gather.copy_positions(view((int32_t)c), rowids, kept, fresh, s);
            cols[c] = std::move(fresh);   // (the old arrays go back to the pool tagged with this stream)
        }
        rows = kept;
    }

    DevColumn view(int32_t channel) const
    {
        const OutColumn& o = cols[(size_t)channel];
        DevColumn c;
        c.type = o.type;
        c.varwidth = o.varwidth;
        c.values = o.values.ptr();
        c.offsets = o.offsets.as<int32_t>();
        c.nulls = o.has_nulls ? o.nulls.as<uint8_t>() : nullptr;
        return c;
    }

    // out_cols[j] = channels[j] of the n rows in the order of perm.  skip (may be null): (*skip)[j] marks a column the caller has
    // produced already, which has no NULLs.  The fixed-width channels and every NULL flag array go through the permutation by ONE
    // launch per GATHER_MULTI_MAX_COLS columns: the permutation is read once, the random reads of all channels are in flight together.
    // A VARCHAR channel's values go through gather.copy_varwidth (its scratch is the caller's, and counted by it).
    void gather_sorted(const int32_t* perm, int64_t n, const std::vector<int32_t>& channels, const std::vector<bool>* skip,
                       std::vector<OutColumn>& out_cols, PositionGather& gather, hipStream_t s) const
    {
        GatherMultiArgs gm;
        memset(&gm, 0, sizeof gm);
        gm.positions[0] = perm;
        gm.count = n;
        auto flush_gather = [&] {
            if (gm.ncols > 0) launch_gather_multi(gm, s);
            gm.ncols = 0;
        };
        for (size_t j = 0; j < channels.size(); j++) {
            const DevColumn h = view(channels[j]);
            OutColumn& oc = out_cols[j];
            oc.type = h.type;
            oc.varwidth = h.varwidth;
            oc.has_nulls = h.nulls != nullptr;
            if (skip && (*skip)[j]) continue;
            if (gm.ncols == GATHER_MULTI_MAX_COLS) flush_gather();
            GatherMultiCol& gc = gm.col[gm.ncols];
            memset(&gc, 0, sizeof gc);
            gc.width = 1;
            // (no 2 GiB message: perm is a permutation of, or distinct rows among, the rows held -- at most INT32_MAX bytes, append_offsets)
            if (h.varwidth) gather.copy_varwidth(h, perm, (int32_t)n, oc.offsets, oc.values, s);
            else {
                const int w = type_width(h.type);   // (1, 4, 8, or 16 for a LONG_DECIMAL: creation refused every other type)
                gc.src = h.values;
                gc.dst = oc.values.ensure((size_t)n * w);
                gc.width = w;
            }
            if (h.nulls) {
                gc.src_nulls = h.nulls;
                gc.dst_nulls = static_cast<uint8_t*>(oc.nulls.ensure((size_t)n));
            }
            if (gc.dst || gc.dst_nulls) gm.ncols++;
        }
        flush_gather();
    }

    size_t bytes() const
    {
        size_t b = 0;
        for (const OutColumn& o : cols) b += o.values.capacity() + o.offsets.capacity() + o.nulls.capacity();
        return b;
    }

    std::vector<OutColumn> cols;      // by input channel
    std::vector<int64_t> var_bytes;   // VARCHAR bytes used
    std::vector<bool> held;
    int64_t rows = 0;
    int64_t reserve_rows = 0;          // room for at least this many rows whenever a column grows (HashBuilder's expected_positions)
    const char* refusal_prefix = "";   // in front of "VARCHAR column exceeds 2 GB" (the join build says whose column)

private:
    int64_t room(int64_t k) const { return std::max(rows + k, reserve_rows); }
    // k offsets (src[0..k], any base) behind the rows held, rebased onto the `add` bytes they bring; returns where those bytes go
    char* append_offsets(size_t c, const int32_t* src, int64_t k, int64_t add, hipStream_t s)
    {
        OutColumn& h = cols[c];
        int64_t& used = var_bytes[c];
        PA_REQUIRE(add >= 0 && used + add <= INT32_MAX, PA_ERR_INSUFFICIENT_RESOURCES, std::string(refusal_prefix) + "VARCHAR column exceeds 2 GB");
        int32_t* off = static_cast<int32_t*>(h.offsets.reserve_keep((size_t)(room(k) + 1) * 4, (size_t)(rows ? rows + 1 : 0) * 4, s));
        launch_offsets_append(src, k, (int32_t)used, off + rows, rows == 0, s);
        char* v = static_cast<char*>(h.values.reserve_keep((size_t)(used + add + 1), (size_t)used, s)) + used;
        used += add;
        return v;
    }
    // the NULL flags of k more rows: where the caller writes the page's flags, or null when it has none (then they are cleared, if the
    // column has flags at all).  The first page with NULLs allocates the array and clears the rows held before it.
    uint8_t* append_nulls(OutColumn& h, bool src_has_nulls, int64_t k, hipStream_t s)
    {
        if (!src_has_nulls && !h.has_nulls) return nullptr;
        uint8_t* nl = static_cast<uint8_t*>(h.nulls.reserve_keep((size_t)room(k), h.has_nulls ? (size_t)rows : 0, s));
        if (!h.has_nulls && rows > 0) PA_HIP(hipMemsetAsync(nl, 0, (size_t)rows, s));
        h.has_nulls = true;
        if (src_has_nulls) return nl + rows;
        PA_HIP(hipMemsetAsync(nl + rows, 0, (size_t)k, s));
        return nullptr;
    }
};

}  // namespace pa

#pragma GCC visibility pop
