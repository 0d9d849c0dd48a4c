// op_window.cpp -- WindowOperator on device, the ranking functions: row_number / rank / dense_rank / percent_rank / cume_dist / ntile
// OVER (PARTITION BY ... ORDER BY ...).
//
// Reference path replaced:
//   LocalExecutionPlanner.visitWindow
//   WindowOperator (…/operator/WindowOperator.java: the sort :294, the partition ends :909-935) over RegularWindowPartition (peer
//   groups :180-190) and RowNumberFunction / RankFunction / DenseRankFunction / PercentRankFunction / CumulativeDistributionFunction /
//   NTileFunction of …/operator/window/.  These six ignore frames; a window node with any other function stays with the reference.
//
// Contract (include/presto_amd.h).  Output only after finish: every input row, sorted by [partition channels ASC_NULLS_LAST] + [sort
// channels], rows that compare equal in arrival order; the output channels, then one column per function.
//
// The operator holds every needed channel of the input, column by column, pages laid behind each other (as OrderBy does).  At the
// first get_output after finish:
//   sort       RowSorter (row_sort.hpp) over partition + sort channels: a permutation, stable, so arrival order inside ties;
//   flags      one launch per channel: IS DISTINCT FROM the sorted row before (window_kernels.hpp) -> partition and peer flags;
//   runs       two exclusive scans number the partitions and the peer groups, one pass stores where each starts;
//   functions  one pass writes every requested column by sorted index; a bad ntile bucket count sets an error word, read back with
//              the scan totals;
//   output     the output channels gathered through the permutation, as OrderBy gathers them.
#include <algorithm>
#include <cstring>

#include "keyed_operator.hpp"
#include "row_sort.hpp"
#include "static_kernels.hpp"
#include "window_kernels.hpp"

namespace pa {
namespace {

bool is_ntile(const pa_window_function_desc& f) { return f.function == PA_WINDOW_NTILE; }

// checked before the device is asked for: a shape the device path does not take is reported as such with or without a GPU
void* checked_stream(const pa_window_desc* d)
{
    PA_REQUIRE(d != nullptr && d->input_types != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    const int32_t channels = d->input_channel_count;
    const int32_t* types = d->input_types;
    check_input_channels(channels);
    PA_REQUIRE(d->function_count >= 1 && d->function_count <= kWindowMaxFunctions && d->functions != nullptr, PA_ERR_INVALID_ARGUMENT, "1..16 window functions");
    PA_REQUIRE(d->output_channel_count >= 0 && (d->output_channel_count == 0 || d->output_channels != nullptr), PA_ERR_INVALID_ARGUMENT, "output channels are null");
    PA_REQUIRE(d->partition_channel_count >= 0 && (d->partition_channel_count == 0 || d->partition_channels != nullptr), PA_ERR_INVALID_ARGUMENT,
               "partition channels are null");
    PA_REQUIRE(d->sort_channel_count >= 0 && (d->sort_channel_count == 0 || (d->sort_channels != nullptr && d->sort_orders != nullptr)), PA_ERR_INVALID_ARGUMENT,
               "sort channels are null");
    check_channels(d->output_channels, d->output_channel_count, channels, "output");
    // (a channel out of range is reported before a count the device path does not take: of a longer list, the first channels only)
    check_channels(d->partition_channels, std::min(d->partition_channel_count, kMaxJoinChannels + 1), channels, "partition");
    for (int32_t i = 0; i < d->sort_channel_count; i++) {
        check_channels(d->sort_channels + i, 1, channels, "sort");
        PA_REQUIRE(d->sort_orders[i] >= 0 && d->sort_orders[i] <= 3, PA_ERR_INVALID_ARGUMENT, "unknown sort order");
    }
    for (int32_t i = 0; i < d->function_count; i++) {
        const pa_window_function_desc& f = d->functions[i];
        PA_REQUIRE(f.function >= PA_WINDOW_ROW_NUMBER && f.function <= PA_WINDOW_NTILE, PA_ERR_INVALID_ARGUMENT, "unknown window function");
        PA_REQUIRE(f.argument_count == (is_ntile(f) ? 1 : 0), PA_ERR_INVALID_ARGUMENT, "wrong number of window function arguments");
        if (!is_ntile(f)) continue;
        PA_REQUIRE(f.argument_channels != nullptr, PA_ERR_INVALID_ARGUMENT, "argument channels are null");
        check_channels(f.argument_channels, 1, channels, "argument");
        const int32_t t = types[f.argument_channels[0]];
        PA_REQUIRE(t == PA_BIGINT || t == PA_INTEGER, PA_ERR_INVALID_ARGUMENT, "ntile takes a BIGINT or INTEGER argument");
    }
    PA_REQUIRE(d->expected_positions >= 0, PA_ERR_INVALID_ARGUMENT, "expected_positions is negative");
    check_output_mem(d->output_mem);
    // what the device path does not take
    PA_REQUIRE(d->pre_grouped_channel_count == 0 && d->pre_sorted_channel_prefix == 0, PA_ERR_NOT_SUPPORTED, "pre-grouped / pre-sorted window input");
    PA_REQUIRE(d->partition_channel_count <= kMaxJoinChannels, PA_ERR_NOT_SUPPORTED, "more partition channels than the device path takes");
    for (int32_t i = 0; i < d->partition_channel_count; i++) check_key_type(types[d->partition_channels[i]], "partition");
    for (int32_t i = 0; i < d->sort_channel_count; i++) check_key_type(types[d->sort_channels[i]], "sort");
    for (int32_t i = 0; i < d->output_channel_count; i++) check_carried_type(types[d->output_channels[i]], "output");
    return d->stream;
}

DevColumn view_of(const OutColumn& o)
{
    DevColumn c;
    c.type = o.type;
    c.varwidth = o.varwidth;
    c.values = o.values.ptr();
    c.offsets = o.offsets.as<int32_t>();
    c.nulls = o.has_nulls ? o.nulls.as<uint8_t>() : nullptr;
    return c;
}

class WindowOperator : public pa_operator {
public:
    explicit WindowOperator(const pa_window_desc* d) : stream_(checked_stream(d))
    {
        types_.assign(d->input_types, d->input_types + d->input_channel_count);
        output_channels_.assign(d->output_channels, d->output_channels + d->output_channel_count);
        // the channels the rows are sorted by: the partition channels ASC_NULLS_LAST, then the sort channels
        for (int32_t i = 0; i < d->partition_channel_count; i++) {
            order_channels_.push_back(d->partition_channels[i]);
            orders_.push_back(PA_ASC_NULLS_LAST);
        }
        partition_count_ = (size_t)d->partition_channel_count;
        for (int32_t i = 0; i < d->sort_channel_count; i++) {
            order_channels_.push_back(d->sort_channels[i]);
            orders_.push_back(d->sort_orders[i]);
        }
        for (int32_t i = 0; i < d->function_count; i++) {
            functions_.push_back(d->functions[i].function);
            argument_channels_.push_back(is_ntile(d->functions[i]) ? d->functions[i].argument_channels[0] : -1);
        }
        output_mem_ = d->output_mem;
        needed_.assign(types_.size(), false);
        for (int32_t c : order_channels_) needed_[c] = true;
        for (int32_t c : output_channels_) needed_[c] = true;
        for (int32_t c : argument_channels_)
            if (c >= 0) needed_[c] = true;
        held_.resize(types_.size());
        held_bytes_.assign(types_.size(), 0);
        for (size_t c = 0; c < types_.size(); c++) {
            held_[c].type = types_[c];
            held_[c].varwidth = types_[c] == PA_VARCHAR;
        }
        timer.set_name("k_window_functions");
    }
    ~WindowOperator() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }

    bool needs_input() override { return !finishing_; }
    bool is_finished() override { return finishing_ && (done_ || rows_ == 0); }
    void finish() override { finishing_ = true; }

    // PagesIndex.addPage: the needed channels of the page behind the rows held so far; its buffers are the caller's again on return
    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(!finishing_, PA_ERR_ILLEGAL_STATE, "Operator is already finishing");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int64_t m = page->position_count;
        if (m <= 0) return;
        PA_REQUIRE(rows_ + m <= INT32_MAX, PA_ERR_INSUFFICIENT_RESOURCES, "more rows held than one sort takes");
        hipStream_t s = stream_.get();
        const DevPage in = stager_.stage(page, &needed_, s);
        for (size_t c = 0; c < types_.size(); c++) {
            if (!needed_[c]) continue;
            const DevColumn& src = in.cols[c];
            PA_REQUIRE(src.type == types_[c], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared input type");
            OutColumn& h = held_[c];
            if (h.varwidth) {
                int32_t ends[2];
                PA_HIP(hipMemcpyAsync(&ends[0], src.offsets, 4, hipMemcpyDeviceToHost, s));
                PA_HIP(hipMemcpyAsync(&ends[1], src.offsets + m, 4, hipMemcpyDeviceToHost, s));
                PA_HIP(hipStreamSynchronize(s));
                const int64_t add = ends[1] - ends[0];
                PA_REQUIRE(add >= 0 && held_bytes_[c] + add <= INT32_MAX, PA_ERR_INSUFFICIENT_RESOURCES, "VARCHAR column exceeds 2 GB");
                int32_t* off = static_cast<int32_t*>(h.offsets.reserve_keep((size_t)(rows_ + m + 1) * 4, (size_t)(rows_ ? rows_ + 1 : 0) * 4, s));
                launch_offsets_append(src.offsets, m, (int32_t)held_bytes_[c], off + rows_, rows_ == 0, s);
                char* v = static_cast<char*>(h.values.reserve_keep((size_t)(held_bytes_[c] + add + 1), (size_t)held_bytes_[c], s));
                if (add) PA_HIP(hipMemcpyAsync(v + held_bytes_[c], static_cast<const char*>(src.values) + ends[0], (size_t)add, hipMemcpyDeviceToDevice, s));
                held_bytes_[c] += add;
            }
            else {
                const size_t w = (size_t)type_width(h.type);
                char* v = static_cast<char*>(h.values.reserve_keep((size_t)(rows_ + m) * w, (size_t)rows_ * w, s));
                PA_HIP(hipMemcpyAsync(v + (size_t)rows_ * w, src.values, (size_t)m * w, hipMemcpyDeviceToDevice, s));
            }
            if (src.nulls || h.has_nulls) {
                uint8_t* nl = static_cast<uint8_t*>(h.nulls.reserve_keep((size_t)(rows_ + m), h.has_nulls ? (size_t)rows_ : 0, s));
                if (!h.has_nulls && rows_ > 0) PA_HIP(hipMemsetAsync(nl, 0, (size_t)rows_, s));
                if (src.nulls) PA_HIP(hipMemcpyAsync(nl + rows_, src.nulls, (size_t)m, hipMemcpyDeviceToDevice, s));
                else PA_HIP(hipMemsetAsync(nl + rows_, 0, (size_t)m, s));
                h.has_nulls = true;
            }
        }
        rows_ += m;
        // the page's buffers are the caller's again, and the stager's are reused by the next page
        PA_HIP(hipStreamSynchronize(s));
    }

    bool get_output(pa_page* out) override
    {
        if (!finishing_ || done_) return false;
        done_ = true;
        if (rows_ == 0) return false;
        hipStream_t s = stream_.get();
        const int32_t n = (int32_t)rows_;
        std::vector<DevColumn> cols;
        for (int32_t c : order_channels_) cols.push_back(view_of(held_[c]));
        const int32_t* perm = sorter_.sort(cols, orders_, nullptr, 0, n, s);
        // runs: flags -> scans -> starts.  flags_: [part_flag | peer_flag | part_index | peer_index], starts_: [part_start | peer_start]
        int32_t* part_flag = static_cast<int32_t*>(flags_.ensure((size_t)n * 16));
        int32_t* peer_flag = part_flag + n;
        int32_t* part_index = peer_flag + n;
        int32_t* peer_index = part_index + n;
        int32_t* part_start = static_cast<int32_t*>(starts_.ensure(((size_t)n + 1) * 8));
        int32_t* peer_start = part_start + (n + (size_t)1);
        int32_t* words = static_cast<int32_t*>(words_.ensure(64));   // [partition flags set, peer flags set, error]
        void* scan_temp = scan_temp_.ensure(scan_temp_bytes(n));
        PA_HIP(hipMemsetAsync(part_flag, 0, (size_t)n * 8, s));
        PA_HIP(hipMemsetAsync(words, 0, 64, s));
        timer.begin(s);
        for (size_t i = 0; i < cols.size(); i++) {
            const DevColumn& c = cols[i];
            const bool partition = i < partition_count_;
            launch_window_distinct(c.type, c.values, c.offsets, c.nulls, perm, n, peer_flag, partition ? part_flag : nullptr, s);
        }
        launch_exclusive_scan_i32(part_flag, part_index, n, words, scan_temp, s);
        launch_exclusive_scan_i32(peer_flag, peer_index, n, words + 1, scan_temp, s);
        launch_window_starts(part_flag, part_index, peer_flag, peer_index, n, part_start, peer_start, s);
        // one column per function, by sorted index
        const size_t nc = output_channels_.size(), nf = functions_.size();
        out_cols_.clear();
        out_cols_.resize(nc + nf);
        WindowFunctionArgs a;
        memset(&a, 0, sizeof a);
        a.perm = perm;
        a.part_flag = part_flag;
        a.part_index = part_index;
        a.peer_flag = peer_flag;
        a.peer_index = peer_index;
        a.part_start = part_start;
        a.peer_start = peer_start;
        a.error = words + 2;
        a.n = n;
        a.count = (int32_t)nf;
        for (size_t k = 0; k < nf; k++) {
            OutColumn& oc = out_cols_[nc + k];
            WindowFunction& f = a.f[k];
            f.function = functions_[k];
            oc.type = f.function == PA_WINDOW_PERCENT_RANK || f.function == PA_WINDOW_CUME_DIST ? PA_DOUBLE : PA_BIGINT;
            f.out = oc.values.ensure((size_t)n * 8);
            if (argument_channels_[k] < 0) continue;
            const OutColumn& arg = held_[argument_channels_[k]];
            f.arg_type = arg.type;
            f.arg_values = arg.values.ptr();
            if (arg.has_nulls) {
                f.arg_nulls = arg.nulls.as<uint8_t>();
                f.out_nulls = static_cast<uint8_t*>(oc.nulls.ensure((size_t)n));
                oc.has_nulls = true;
            }
        }
        launch_window_functions(a, s);
        timer.end(s);
        int32_t h_words[3] = {0, 0, 0};
        read_back(h_words, words, sizeof h_words, s);
        PA_REQUIRE(h_words[0] >= 0 && h_words[0] <= h_words[1] && h_words[1] < n, PA_ERR_DEVICE, "window: run counts out of range");
        PA_REQUIRE(h_words[2] == 0, PA_ERR_INVALID_ARGUMENT, "Buckets must be greater than 0");
        gather_output(perm, n, s);
        publish_output(out_cols_, n, output_mem_, s, out, storage_);
        return true;
    }

    void close() override { (void)hipStreamSynchronize(stream_.get()); }

    // the rows held, and the scratch of the sort and the passes while it is allocated
    int64_t memory_bytes() override
    {
        size_t b = stager_.bytes() + sorter_.bytes() + flags_.capacity() + starts_.capacity() + words_.capacity() + scan_temp_.capacity();
        for (const OutColumn& o : held_) b += o.values.capacity() + o.offsets.capacity() + o.nulls.capacity();
        return (int64_t)b;
    }

private:
    // the output channels in sorted order (PagesIndex.appendTo): the fixed-width channels and every NULL flag array through the
    // permutation by one launch per 24 columns, a VARCHAR channel by lengths -> scan -> copy
    void gather_output(const int32_t* perm, int32_t n, hipStream_t s)
    {
        GatherMultiArgs gm;
        memset(&gm, 0, sizeof gm);
        gm.positions[0] = perm;
        gm.count = n;
        auto flush_gather = [&] {
            if (gm.ncols > 0) launch_gather_multi(gm, s);
            gm.ncols = 0;
        };
        for (size_t j = 0; j < output_channels_.size(); j++) {
            const OutColumn& h = held_[output_channels_[j]];
            OutColumn& oc = out_cols_[j];
            oc.type = h.type;
            oc.varwidth = h.varwidth;
            const uint8_t* nulls = h.has_nulls ? h.nulls.as<uint8_t>() : nullptr;
            oc.has_nulls = nulls != nullptr;
            if (gm.ncols == GATHER_MULTI_MAX_COLS) flush_gather();
            GatherMultiCol& gc = gm.col[gm.ncols];
            memset(&gc, 0, sizeof gc);
            gc.width = 1;
            if (h.varwidth) {
                int32_t* lens = static_cast<int32_t*>(oc.offsets.ensure(((size_t)n + 1) * 4));
                int32_t* total = static_cast<int32_t*>(words_.ensure(64)) + 4;
                launch_varwidth_lengths(perm, n, h.offsets.as<int32_t>(), nulls, lens, s);
                launch_exclusive_scan_i32(lens, lens, n, total, scan_temp_.ensure(scan_temp_bytes(n)), s);
                int32_t h_total = 0;
                read_back(&h_total, total, 4, s);
                launch_varwidth_copy(perm, n, h.offsets.as<int32_t>(), h.values.as<uint8_t>(), nulls, lens,
                                     static_cast<uint8_t*>(oc.values.ensure((size_t)(h_total > 0 ? h_total : 1))), total, s);
            }
            else {
                const int w = type_width(h.type);   // (1, 4, 8, or 16 for a LONG_DECIMAL: creation refused every other type)
                gc.src = h.values.ptr();
                gc.dst = oc.values.ensure((size_t)n * w);
                gc.width = w;
            }
            if (nulls) {
                gc.src_nulls = nulls;
                gc.dst_nulls = static_cast<uint8_t*>(oc.nulls.ensure((size_t)n));
            }
            if (gc.dst || gc.dst_nulls) gm.ncols++;
        }
        flush_gather();
    }

    Stream stream_;
    PageStager stager_;
    std::vector<int32_t> types_, output_channels_, order_channels_, orders_, functions_, argument_channels_;
    size_t partition_count_ = 0;   // the first of order_channels_ are the partition channels
    std::vector<bool> needed_;
    int32_t output_mem_ = PA_MEM_HOST;
    // the rows held, by input channel
    std::vector<OutColumn> held_;
    std::vector<int64_t> held_bytes_;   // VARCHAR bytes used
    int64_t rows_ = 0;
    RowSorter sorter_;
    DevBuf flags_, starts_, words_, scan_temp_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> storage_;
    bool finishing_ = false, done_ = false;
};

}  // namespace

pa_operator* make_window(const pa_window_desc* desc) { return new WindowOperator(desc); }

}  // namespace pa
