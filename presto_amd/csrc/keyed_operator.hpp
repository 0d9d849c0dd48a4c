// keyed_operator.hpp -- what the operators over a key table share on the host: MarkDistinct / DistinctLimit (op_distinct.cpp),
// SetBuilder / HashSemiJoin (op_semi_join.cpp), RowNumber (op_row_number.cpp), TopNRanking (op_topn_ranking.cpp).  The type checks
// also serve the operators that sort, join or collect by a channel (op_order_by.cpp, op_topn.cpp, op_join.cpp, op_dynamic_filter.cpp).
//
//   descriptor checks    check_key_type, check_carried_type, check_input_channels, check_channels, check_key_channels, check_hash_channel, check_output_mem
//   the key table        make_distinct_hash, KeyColumns, bits_for, grow_by_group_id
//   KeepCompactor        keep marks -> rows kept per block -> scan -> positions (one read-back)
//   PassThroughOutput    "the input page's channels with one computed column behind them": the retained input page, the zero-copy
//                        output page over the caller's own blocks, the views of the staged columns otherwise
// The state machines of the operators differ and stay written out in each of them: these are members and free functions, not a base.
#pragma once

#include <deque>
#include <string>

#include "distinct_hash.hpp"
#include "operator.hpp"
#include "position_gather.hpp"
#include "row_number_kernels.hpp"

// (internal to the library: the inline functions and classes here stay out of its exported symbols)
#pragma GCC visibility push(hidden)

namespace pa {

// ---- descriptor checks: before the device is asked for, so a shape the device path does not take is reported as such with or
// without a GPU.  Where a descriptor has two defects the first check decides the status: every operator keeps its own order. -----------
// the key types the canonical 64-bit word covers (kernels/pa_canon.h) -- also the types with an order-preserving image
// (topn_kernels.hip), a join equality (join_kernels.hip) and a dynamic-filter key; `what`: "distinct", "partition", "semi-join", "sort", "join"
inline void check_key_type(int32_t type, const char* what)
{
    switch (type) {
        case PA_BIGINT:
        case PA_INTEGER:
        case PA_DATE:
        case PA_DOUBLE:
        case PA_REAL:
        case PA_BOOLEAN:
        case PA_VARCHAR:
        case PA_DECIMAL: return;
        case PA_LONG_DECIMAL:
        case PA_ROW: throw Error(PA_ERR_NOT_SUPPORTED, std::string(what) + " key type not supported on the device");
        default: throw Error(PA_ERR_INVALID_ARGUMENT, std::string("unknown ") + what + " key type");
    }
}
// a channel an operator only carries -- copied position by position, never compared or hashed: every flat or variable-width type
// (LONG_DECIMAL as 16-byte elements); `what`: "output", "payload", "pass-through"
inline void check_carried_type(int32_t type, const char* what)
{
    switch (type) {
        case PA_BIGINT:
        case PA_INTEGER:
        case PA_DATE:
        case PA_DOUBLE:
        case PA_REAL:
        case PA_BOOLEAN:
        case PA_VARCHAR:
        case PA_DECIMAL:
        case PA_LONG_DECIMAL: return;
        case PA_ROW: throw Error(PA_ERR_NOT_SUPPORTED, std::string(what) + " channel type not supported on the device");
        default: throw Error(PA_ERR_INVALID_ARGUMENT, std::string("unknown ") + what + " channel type");
    }
}
inline void check_input_channels(int32_t channels) { PA_REQUIRE(channels > 0 && channels <= 64, PA_ERR_NOT_SUPPORTED, "1..64 input channels"); }
// the first `count` entries of a channel list are input channels
inline void check_channels(const int32_t* list, int32_t count, int32_t channels, const char* what)
{
    for (int32_t i = 0; i < count; i++) PA_REQUIRE(list[i] >= 0 && list[i] < channels, PA_ERR_INVALID_ARGUMENT, std::string(what) + " channel out of range");
}
// key channels one by one: an input channel, then of a key type
inline void check_key_channels(const int32_t* list, int32_t count, int32_t channels, const int32_t* types, const char* what)
{
    for (int32_t i = 0; i < count; i++) {
        check_channels(list + i, 1, channels, what);
        check_key_type(types[list[i]], what);
    }
}
// a $hashvalue channel is accepted and not read
inline void check_hash_channel(int32_t hash_channel, int32_t channels, const int32_t* types)
{
    PA_REQUIRE(hash_channel >= -1 && hash_channel < channels, PA_ERR_INVALID_ARGUMENT, "hash channel out of range");
    PA_REQUIRE(hash_channel < 0 || types[hash_channel] == PA_BIGINT, PA_ERR_INVALID_ARGUMENT, "hash channel must be BIGINT");
}
inline void check_output_mem(int32_t output_mem)
{
    PA_REQUIRE(output_mem == PA_MEM_HOST || output_mem == PA_MEM_DEVICE, PA_ERR_INVALID_ARGUMENT, "unknown output_mem");
}

// ---- the key table ------------------------------------------------------------------------------------------------------------------
// the table over the key channels of an operator (null: no key channels -- one group, no table)
inline std::unique_ptr<DistinctHash> make_distinct_hash(const std::vector<int32_t>& types, const std::vector<int32_t>& channels, int32_t expected, hipStream_t s)
{
    if (channels.empty()) return nullptr;
    std::vector<int32_t> key_types;
    for (int32_t c : channels) key_types.push_back(types[c]);
    return std::unique_ptr<DistinctHash>(new DistinctHash(key_types, expected, s));
}

// the key columns of a staged page, as DistinctHash::add_page takes them
struct KeyColumns {
    KeyColumns(const DevPage& in, const std::vector<int32_t>& channels)
    {
        for (size_t i = 0; i < channels.size(); i++) cols[i] = &in.cols[channels[i]];
    }
    const DevColumn* cols[kMaxJoinChannels];
};

// the bits a sort of group ids below `count` has to look at
inline int bits_for(int64_t count)
{
    int b = 1;
    while (((int64_t)1 << b) < count) b++;
    return b;
}

// an array of 8-byte entries by group id grows with the key store: at least doubled, the new entries filled with the byte `fill`
inline void grow_by_group_id(DevBuf& buf, int64_t* entries, int64_t groups, int fill, hipStream_t s)
{
    if (groups <= *entries) return;
    const int64_t want = std::max<int64_t>(std::max<int64_t>(groups, 2 * *entries), 1024);
    buf.reserve_keep((size_t)want * 8, (size_t)*entries * 8, s);
    PA_HIP(hipMemsetAsync(buf.as<char>() + (size_t)*entries * 8, fill, (size_t)(want - *entries) * 8, s));
    *entries = want;
}

// ---- keep marks -> positions ----------------------------------------------------------------------------------------------------------
// The rows kept of a page (or of the held rows), compacted in input order: the keep passes of row_number_kernels.hpp around the scan.
// The count of rows kept comes back to the host: the one read-back of a call.
struct KeepCompactor {
    // keep: round_up(n, 4) bytes, the n first written; returns the positions (null when *kept == 0).  `what` names the operator in the error
    const int32_t* positions_of(const uint8_t* keep, int32_t n, int32_t* kept, const char* what, hipStream_t s)
    {
        const int64_t blocks = row_number_blocks(n);
        int32_t* counts = static_cast<int32_t*>(block_counts.ensure((size_t)blocks * 4));
        int32_t* d_total = static_cast<int32_t*>(total.ensure(64));
        launch_row_number_keep_counts(keep, n, counts, s);
        launch_exclusive_scan_i32(counts, counts, blocks, d_total, scan_temp.ensure(scan_temp_bytes(blocks)), s);
        int32_t h_total = 0;
        read_back(&h_total, d_total, 4, s);
        PA_REQUIRE(h_total >= 0 && h_total <= n, PA_ERR_DEVICE, std::string(what) + ": kept rows out of range");
        *kept = h_total;
        if (h_total == 0) return nullptr;
        int32_t* p = static_cast<int32_t*>(positions.ensure((size_t)h_total * 4));
        launch_row_number_keep_positions(keep, n, counts, p, s);
        return p;
    }
    size_t bytes() const { return positions.capacity() + block_counts.capacity() + scan_temp.capacity() + total.capacity(); }
    // (scan_temp and total also serve the other scans of an operator between two calls)
    DevBuf positions, block_counts, scan_temp, total;
};

// ---- the pass-through output page --------------------------------------------------------------------------------------------------------
inline std::vector<int32_t> all_channels(size_t n)
{
    std::vector<int32_t> all(n);
    for (size_t c = 0; c < n; c++) all[c] = (int32_t)c;
    return all;
}

// Output page = channels of the input page + one computed flat column (Page.appendColumn).  A device page into a device-output operator
// goes out as the caller's own blocks, encodings included (zero copy): only the key channels are staged, and a PA_PAGE_RETAINED page must
// outlive the output page.  So the operator (takes_retained() = true) calls
//   release()  where nothing reads the last page any more: needs_input / get_output without a pending output, at the top of add_input,
//              in close and in its destructor;
//   hold()     right behind that release() in add_input, before any check can throw: a page handed over is let go whatever happens;
//   stage()    for a page with rows, publish() for its output page.
class PassThroughOutput {
public:
    // channels: the input channels that go out, in output order; keys: the channels the operator reads itself
    void init(size_t input_channels, const std::vector<int32_t>& channels, const std::vector<int32_t>& keys, int32_t output_mem)
    {
        channels_ = channels;
        output_mem_ = output_mem;
        key_only_.assign(input_channels, false);
        needed_.assign(input_channels, false);
        for (int32_t c : keys) key_only_[c] = needed_[c] = true;
        for (int32_t c : channels) needed_[c] = true;
    }
    void hold(const pa_page* page)
    {
        if (page != nullptr && (page->flags & PA_PAGE_RETAINED) != 0 && page->release != nullptr) held_ = {page->release, page->release_ctx};
    }
    // idempotent; the stream is drained first, and only when a page is held
    void release(hipStream_t s)
    {
        if (held_.fn == nullptr) return;
        (void)hipStreamSynchronize(s);
        const Release r = held_;
        held_ = {nullptr, nullptr};
        r.fn(r.ctx);
    }

    // The page on the device.  Zero copy (when the caller allows it and the page and the output both live in HBM): the key channels only,
    // and the caller's pa_column structs of the output channels copied with their dictionaries -- they are the caller's own again when
    // add_input returns.  Else every channel the operator reads or emits.
    const DevPage& stage(PageStager& stager, const pa_page* page, bool allow_zero_copy, hipStream_t s)
    {
        zero_copy_ = allow_zero_copy && page->mem == PA_MEM_DEVICE && output_mem_ == PA_MEM_DEVICE;
        in_ = stager.stage(page, zero_copy_ ? &key_only_ : &needed_, s);
        if (zero_copy_) {
            dict_copies_.clear();
            storage_.resize(channels_.size() + 1);
            for (size_t c = 0; c < channels_.size(); c++) storage_[c] = copy_column(page->columns[channels_[c]]);
        }
        return in_;
    }

    // the output page of the page staged last: its n rows, the computed column (`nulls` may be null) behind the channels
    void publish(int32_t n, int32_t type, const void* values, const uint8_t* nulls, hipStream_t s, pa_page* out)
    {
        const size_t nc = channels_.size();
        if (zero_copy_) {
            pa_column& m = storage_[nc];
            memset(&m, 0, sizeof m);
            m.type = type;
            m.encoding = PA_FLAT;
            m.values = values;
            m.nulls = nulls;
            out->position_count = n;
            out->channel_count = (int32_t)nc + 1;
            out->columns = storage_.data();
            out->mem = PA_MEM_DEVICE;
            out->flags = 0;
            out->release = nullptr;
            out->release_ctx = nullptr;
            return;
        }
        out_cols_.resize(nc + 1);
        for (size_t c = 0; c < nc; c++) view_column(out_cols_[c], in_.cols[channels_[c]]);
        DevColumn computed;
        computed.type = type;
        computed.values = values;
        computed.nulls = nulls;
        view_column(out_cols_[nc], computed);
        publish_output(out_cols_, n, output_mem_, s, out, storage_);
    }

private:
    struct Release {
        void (*fn)(void*);
        void* ctx;
    };
    // a block of the input page, its dictionary (DICTIONARY / RLE / ROW_FIELDS) copied
    pa_column copy_column(const pa_column& c)
    {
        pa_column o = c;
        if (c.dictionary != nullptr && (c.encoding == PA_DICTIONARY || c.encoding == PA_RLE || c.encoding == PA_ROW_FIELDS)) {
            const int32_t k = c.encoding == PA_ROW_FIELDS ? c.dictionary_size : 1;
            dict_copies_.emplace_back(std::max(k, 1));
            std::vector<pa_column>& held = dict_copies_.back();
            for (int32_t i = 0; i < k; i++) held[i] = copy_column(c.dictionary[i]);
            o.dictionary = held.data();
        }
        return o;
    }

    std::vector<int32_t> channels_;
    std::vector<bool> key_only_, needed_;
    int32_t output_mem_ = PA_MEM_HOST;
    DevPage in_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> storage_;
    std::deque<std::vector<pa_column>> dict_copies_;
    Release held_{nullptr, nullptr};
    bool zero_copy_ = false;
};

}  // namespace pa

#pragma GCC visibility pop
