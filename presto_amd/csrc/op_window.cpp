// op_window.cpp -- WindowOperator on device: the ranking functions row_number / rank / dense_rank / percent_rank / cume_dist / ntile and,
// through the framed descriptor, count / sum / min / max and lag / lead / first_value / last_value / nth_value over the frames that
// start at UNBOUNDED PRECEDING, OVER (PARTITION BY ... ORDER BY ...).
//
// Reference path replaced:
//   LocalExecutionPlanner.visitWindow
//   WindowOperator (…/operator/WindowOperator.java: the sort :294, the partition ends :909-935) over RegularWindowPartition (peer
//   groups :180-190) and RowNumberFunction / RankFunction / DenseRankFunction / PercentRankFunction / CumulativeDistributionFunction /
//   NTileFunction of …/operator/window/, which ignore frames; AggregateWindowFunction over CountAggregation / CountColumn /
//   LongSumAggregation / the min and max of AbstractMinMaxAggregationFunction; LagFunction / LeadFunction / FirstValueFunction /
//   LastValueFunction / NthValueFunction.  A window node with any other function or frame, IGNORE NULLS or a VARCHAR value stays with
//   the reference.
//
// Contract (include/presto_amd.h).  Output only after finish: every input row, sorted by [partition channels ASC_NULLS_LAST] + [sort
// channels], rows that compare equal in arrival order; the output channels, then one column per function.
//
// The operator holds every needed channel of the input in a HeldRows (held_rows.hpp), as OrderBy does.  At the
// first get_output after finish:
//   sort       RowSorter (row_sort.hpp) over partition + sort channels: a permutation, stable, so arrival order inside ties;
//   flags      one launch per channel: IS DISTINCT FROM the sorted row before (window_kernels.hpp) -> partition and peer flags;
//   runs       two exclusive scans number the partitions and the peer groups, one pass stores where each starts;
//   aggregates per distinct argument channel one gather into sorted order; per distinct (kind, channel) one segmented scan;
//   functions  one pass writes every requested column by sorted index: a value column copies its value channel's bytes from the held
//              row at perm[target]; a bad ntile bucket count, a sum outside int64 and a bad lag / lead / nth_value offset set bits of
//              an error word, read back with the scan totals;
//   output     the output channels gathered through the permutation, as OrderBy gathers them.
#include <algorithm>
#include <cstring>

#include "held_rows.hpp"
#include "keyed_operator.hpp"
#include "row_sort.hpp"
#include "static_kernels.hpp"
#include "window_kernels.hpp"

namespace pa {
namespace {

bool is_aggregate(int32_t function) { return function >= PA_WINDOW_COUNT_STAR && function <= PA_WINDOW_MAX; }
bool is_value(int32_t function) { return function >= PA_WINDOW_LAG && function <= PA_WINDOW_NTH_VALUE; }
bool is_shift(int32_t function) { return function == PA_WINDOW_LAG || function == PA_WINDOW_LEAD; }
int32_t min_arguments_of(int32_t function)
{
    if (function == PA_WINDOW_NTH_VALUE) return 2;
    return function == PA_WINDOW_NTILE || is_value(function) || (is_aggregate(function) && function != PA_WINDOW_COUNT_STAR) ? 1 : 0;
}
int32_t max_arguments_of(int32_t function) { return is_shift(function) ? 3 : min_arguments_of(function); }

// One window function as the operator runs it, whichever descriptor it came from.
struct FunctionSpec {
    int32_t function;
    int32_t argument_channel;   // -1: none; a value function: the value channel
    int32_t offset_channel;     // lag / lead / nth_value; -1: none
    int32_t default_channel;    // lag / lead; -1: none
    int32_t frame_end;          // aggregates, first_value / last_value / nth_value: WindowFrameEnd
};

// ---- the two function descriptors: what is an invalid argument, what is refused, what the operator keeps ------------------------------
int32_t last_function(const pa_window_function_desc&) { return PA_WINDOW_NTILE; }
int32_t last_function(const pa_framed_window_function_desc&) { return PA_WINDOW_NTH_VALUE; }

void check_frame_arguments(const pa_window_function_desc&, int32_t) {}
void check_frame_arguments(const pa_framed_window_function_desc& f, int32_t channels)
{
    PA_REQUIRE(f.frame_type >= PA_FRAME_RANGE && f.frame_type <= PA_FRAME_GROUPS, PA_ERR_INVALID_ARGUMENT, "unknown frame type");
    PA_REQUIRE(f.start_type >= PA_BOUND_UNBOUNDED_PRECEDING && f.start_type <= PA_BOUND_UNBOUNDED_FOLLOWING, PA_ERR_INVALID_ARGUMENT, "unknown frame start");
    PA_REQUIRE(f.end_type >= PA_BOUND_UNBOUNDED_PRECEDING && f.end_type <= PA_BOUND_UNBOUNDED_FOLLOWING, PA_ERR_INVALID_ARGUMENT, "unknown frame end");
    PA_REQUIRE(f.start_type != PA_BOUND_UNBOUNDED_FOLLOWING, PA_ERR_INVALID_ARGUMENT, "a frame cannot start at UNBOUNDED FOLLOWING");
    PA_REQUIRE(f.end_type != PA_BOUND_UNBOUNDED_PRECEDING, PA_ERR_INVALID_ARGUMENT, "a frame cannot end at UNBOUNDED PRECEDING");
    if (f.start_type == PA_BOUND_PRECEDING || f.start_type == PA_BOUND_FOLLOWING) check_channels(&f.start_channel, 1, channels, "frame start");
    if (f.end_type == PA_BOUND_PRECEDING || f.end_type == PA_BOUND_FOLLOWING) check_channels(&f.end_channel, 1, channels, "frame end");
    if (is_value(f.function)) PA_REQUIRE(f.ignore_nulls == 0 || f.ignore_nulls == 1, PA_ERR_INVALID_ARGUMENT, "ignore_nulls is 0 or 1");
    else PA_REQUIRE(f.ignore_nulls == 0, PA_ERR_INVALID_ARGUMENT, "IGNORE NULLS is not taken");
}
bool ignore_nulls_of(const pa_window_function_desc&) { return false; }
bool ignore_nulls_of(const pa_framed_window_function_desc& f) { return f.ignore_nulls != 0; }

// (the frames the device path takes are a prefix of the partition; -1: another frame)
int32_t frame_end_of(const pa_window_function_desc&) { return kWindowFramePartition; }
int32_t frame_end_of(const pa_framed_window_function_desc& f)
{
    if (f.start_type != PA_BOUND_UNBOUNDED_PRECEDING) return -1;
    if (f.end_type == PA_BOUND_UNBOUNDED_FOLLOWING) return kWindowFramePartition;
    if (f.end_type != PA_BOUND_CURRENT_ROW) return -1;
    return f.frame_type == PA_FRAME_ROWS ? kWindowFrameRow : kWindowFramePeers;
}

// (params: the channels' type parameters, or null = all 0)
template <class F>
void check_function_arguments(const F& f, int32_t channels, const int32_t* types, const int32_t* params)
{
    PA_REQUIRE(f.function >= PA_WINDOW_ROW_NUMBER && f.function <= last_function(f), PA_ERR_INVALID_ARGUMENT, "unknown window function");
    check_frame_arguments(f, channels);
    PA_REQUIRE(f.argument_count >= min_arguments_of(f.function) && f.argument_count <= max_arguments_of(f.function), PA_ERR_INVALID_ARGUMENT,
               "wrong number of window function arguments");
    if (f.argument_count == 0) return;
    PA_REQUIRE(f.argument_channels != nullptr, PA_ERR_INVALID_ARGUMENT, "argument channels are null");
    check_channels(f.argument_channels, f.argument_count, channels, "argument");
    const int32_t t = types[f.argument_channels[0]];
    if (f.function == PA_WINDOW_NTILE) PA_REQUIRE(t == PA_BIGINT || t == PA_INTEGER, PA_ERR_INVALID_ARGUMENT, "ntile takes a BIGINT or INTEGER argument");
    if (f.function == PA_WINDOW_SUM) PA_REQUIRE(t != PA_VARCHAR && t != PA_BOOLEAN && t != PA_DATE, PA_ERR_INVALID_ARGUMENT, "sum takes a numeric argument");
    if (!is_value(f.function)) return;
    if (f.argument_count >= 2) {
        const int32_t o = types[f.argument_channels[1]];
        PA_REQUIRE(o == PA_BIGINT || o == PA_INTEGER, PA_ERR_INVALID_ARGUMENT, "a window function offset is BIGINT or INTEGER");
    }
    if (f.argument_count >= 3) {
        const int32_t v = f.argument_channels[0], d = f.argument_channels[2];
        const bool parametrised = t == PA_DECIMAL || t == PA_LONG_DECIMAL;
        PA_REQUIRE(types[d] == t && (!parametrised || params == nullptr || params[d] == params[v]), PA_ERR_INVALID_ARGUMENT,
                   "the default of lag / lead has the value's type");
    }
}

// what the device path does not take of a function that is well formed
template <class F>
void check_function_supported(const F& f, const int32_t* types)
{
    if (is_value(f.function)) {
        const int32_t t = types[f.argument_channels[0]];
        PA_REQUIRE(!ignore_nulls_of(f), PA_ERR_NOT_SUPPORTED, "IGNORE NULLS");
        PA_REQUIRE(t != PA_VARCHAR, PA_ERR_NOT_SUPPORTED, "a value window function over a VARCHAR argument");
        check_carried_type(t, "value function argument");
        if (is_shift(f.function)) return;   // (the frame is not read)
    }
    else if (!is_aggregate(f.function)) return;
    PA_REQUIRE(frame_end_of(f) >= 0, PA_ERR_NOT_SUPPORTED, "window frame outside UNBOUNDED PRECEDING .. CURRENT ROW / UNBOUNDED FOLLOWING");
    if (is_value(f.function)) return;
    if (f.function == PA_WINDOW_COUNT_STAR) return;
    const int32_t t = types[f.argument_channels[0]];
    if (f.function == PA_WINDOW_COUNT) check_carried_type(t, "count argument");
    else if (f.function == PA_WINDOW_SUM) {
        check_carried_type(t, "sum argument");
        PA_REQUIRE(t == PA_BIGINT || t == PA_INTEGER, PA_ERR_NOT_SUPPORTED, "sum over a floating-point or DECIMAL argument");
    }
    else {
        check_carried_type(t, "min / max argument");
        PA_REQUIRE(t != PA_VARCHAR && t != PA_LONG_DECIMAL, PA_ERR_NOT_SUPPORTED, "min / max over a VARCHAR or long decimal argument");
    }
}

template <class F>
FunctionSpec spec_of(const F& f)
{
    auto channel = [&f](int32_t k) { return f.argument_count > k ? f.argument_channels[k] : -1; };
    return FunctionSpec{f.function, channel(0), channel(1), channel(2), frame_end_of(f)};
}

// checked before the device is asked for: a shape the device path does not take is reported as such with or without a GPU
// (Desc: pa_window_desc or pa_framed_window_desc, the same fields around their own function descriptors)
template <class Desc>
void* checked_stream(const Desc* d)
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
    for (int32_t i = 0; i < d->function_count; i++) check_function_arguments(d->functions[i], channels, types, d->input_type_params);
    PA_REQUIRE(d->expected_positions >= 0, PA_ERR_INVALID_ARGUMENT, "expected_positions is negative");
    check_output_mem(d->output_mem);
    // what the device path does not take
    PA_REQUIRE(d->pre_grouped_channel_count == 0 && d->pre_sorted_channel_prefix == 0, PA_ERR_NOT_SUPPORTED, "pre-grouped / pre-sorted window input");
    PA_REQUIRE(d->partition_channel_count <= kMaxJoinChannels, PA_ERR_NOT_SUPPORTED, "more partition channels than the device path takes");
    for (int32_t i = 0; i < d->partition_channel_count; i++) check_key_type(types[d->partition_channels[i]], "partition");
    for (int32_t i = 0; i < d->sort_channel_count; i++) check_key_type(types[d->sort_channels[i]], "sort");
    for (int32_t i = 0; i < d->output_channel_count; i++) check_carried_type(types[d->output_channels[i]], "output");
    for (int32_t i = 0; i < d->function_count; i++) check_function_supported(d->functions[i], types);
    return d->stream;
}

size_t round_up_256(size_t b) { return (b + 255) & ~(size_t)255; }

class WindowOperator : public pa_operator {
public:
    template <class Desc>
    explicit WindowOperator(const Desc* d) : stream_(checked_stream(d))
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
        for (int32_t i = 0; i < d->function_count; i++) functions_.push_back(spec_of(d->functions[i]));
        output_mem_ = d->output_mem;
        needed_.assign(types_.size(), false);
        for (int32_t c : order_channels_) needed_[c] = true;
        for (int32_t c : output_channels_) needed_[c] = true;
        for (const FunctionSpec& f : functions_)
            for (int32_t c : {f.argument_channel, f.offset_channel, f.default_channel})
                if (c >= 0) needed_[c] = true;
        held_.init(types_, needed_);
        timer.set_name("k_window_functions");
    }
    ~WindowOperator() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }

    bool needs_input() override { return !finishing_; }
    bool is_finished() override { return finishing_ && (done_ || held_.rows == 0); }
    void finish() override { finishing_ = true; }

    // PagesIndex.addPage: the needed channels of the page behind the rows held so far; its buffers are the caller's again on return
    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(!finishing_, PA_ERR_ILLEGAL_STATE, "Operator is already finishing");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int64_t m = page->position_count;
        if (m <= 0) return;
        PA_REQUIRE(held_.rows + m <= INT32_MAX, PA_ERR_INSUFFICIENT_RESOURCES, "more rows held than one sort takes");
        hipStream_t s = stream_.get();
        const DevPage in = stager_.stage(page, &needed_, s);
        held_.append_page(in, m, s);
        // the page's buffers are the caller's again, and the stager's are reused by the next page
        PA_HIP(hipStreamSynchronize(s));
    }

    bool get_output(pa_page* out) override
    {
        if (!finishing_ || done_) return false;
        done_ = true;
        if (held_.rows == 0) return false;
        hipStream_t s = stream_.get();
        const int32_t n = (int32_t)held_.rows;
        std::vector<DevColumn> cols;
        for (int32_t c : order_channels_) cols.push_back(held_.view(c));
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
        const std::vector<AggregateScan> scans = run_aggregate_scans(perm, part_flag, n, words + 2, s);
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
            const FunctionSpec& spec = functions_[k];
            f.function = spec.function;
            f.frame_end = spec.frame_end;
            const bool min_max = spec.function == PA_WINDOW_MIN || spec.function == PA_WINDOW_MAX;
            const bool value = is_value(spec.function);
            oc.type = min_max || value ? types_[spec.argument_channel]
                              : spec.function == PA_WINDOW_PERCENT_RANK || spec.function == PA_WINDOW_CUME_DIST ? PA_DOUBLE : PA_BIGINT;
            f.out = oc.values.ensure((size_t)n * (size_t)type_width(oc.type));
            if (spec.argument_channel < 0) continue;
            const OutColumn& arg = held_.cols[spec.argument_channel];
            f.arg_type = arg.type;
            if (value) {
                // the value channel by held row at its own width; offset and default at the current row
                f.width = type_width(oc.type);
                f.arg_values = arg.values.ptr();
                if (arg.has_nulls) f.arg_nulls = arg.nulls.as<uint8_t>();
                if (spec.offset_channel >= 0) {
                    const OutColumn& offset = held_.cols[spec.offset_channel];
                    f.offset_type = offset.type;
                    f.offset_values = offset.values.ptr();
                    if (offset.has_nulls) f.offset_nulls = offset.nulls.as<uint8_t>();
                }
                if (spec.default_channel >= 0) {
                    const OutColumn& fallback = held_.cols[spec.default_channel];
                    f.default_values = fallback.values.ptr();
                    if (fallback.has_nulls) f.default_nulls = fallback.nulls.as<uint8_t>();
                }
                // first_value / last_value over a channel without NULLs never give NULL
                if (!arg.has_nulls && (spec.function == PA_WINDOW_FIRST_VALUE || spec.function == PA_WINDOW_LAST_VALUE)) continue;
            }
            else if (is_aggregate(spec.function)) {
                // (count over a channel without NULLs needs no scan: it is the frame's size)
                f.count = static_cast<const int32_t*>(scan_of(scans, kWindowScanCount, spec.argument_channel));
                if (spec.function == PA_WINDOW_COUNT) continue;
                f.scan = scan_of(scans, scan_kind_of(spec.function), spec.argument_channel);
                if (f.count == nullptr) continue;
            }
            else {
                f.arg_values = arg.values.ptr();
                if (!arg.has_nulls) continue;
                f.arg_nulls = arg.nulls.as<uint8_t>();
            }
            f.out_nulls = static_cast<uint8_t*>(oc.nulls.ensure((size_t)n));
            oc.has_nulls = true;
        }
        launch_window_functions(a, s);
        timer.end(s);
        int32_t h_words[3] = {0, 0, 0};
        read_back(h_words, words, sizeof h_words, s);
        PA_REQUIRE(h_words[0] >= 0 && h_words[0] <= h_words[1] && h_words[1] < n, PA_ERR_DEVICE, "window: run counts out of range");
        PA_REQUIRE((h_words[2] & kWindowErrorBuckets) == 0, PA_ERR_INVALID_ARGUMENT, "Buckets must be greater than 0");
        PA_REQUIRE((h_words[2] & kWindowErrorSum) == 0, PA_ERR_NUMERIC_VALUE_OUT_OF_RANGE, "bigint addition overflow in a window sum");
        PA_REQUIRE((h_words[2] & kWindowErrorLagOffset) == 0, PA_ERR_INVALID_ARGUMENT, "Offset must be at least 0");
        PA_REQUIRE((h_words[2] & kWindowErrorNthOffset) == 0, PA_ERR_INVALID_ARGUMENT, "Offset must be at least 1");
        // the output channels in sorted order (PagesIndex.appendTo)
        held_.gather_sorted(perm, n, output_channels_, nullptr, out_cols_, gather_, s);
        publish_output(out_cols_, n, output_mem_, s, out, storage_);
        return true;
    }

    void close() override { (void)hipStreamSynchronize(stream_.get()); }

    // the rows held, and the scratch of the sort and the passes while it is allocated
    int64_t memory_bytes() override
    {
        size_t b = stager_.bytes() + sorter_.bytes() + flags_.capacity() + starts_.capacity() + words_.capacity() + scan_temp_.capacity() + aggregates_.capacity() + gather_.bytes();
        return (int64_t)(b + held_.bytes());
    }

private:
    // a scanned state by sorted index: (count, channel) -> int32 per row, (sum / min / max, channel) -> 8 bytes per row
    struct AggregateScan {
        int32_t kind, channel;
        const void* out;
    };
    static int32_t scan_kind_of(int32_t function)
    {
        return function == PA_WINDOW_SUM ? kWindowScanSum : function == PA_WINDOW_MIN ? kWindowScanMin : function == PA_WINDOW_MAX ? kWindowScanMax : kWindowScanCount;
    }
    static const AggregateScan* find_scan(const std::vector<AggregateScan>& scans, int32_t kind, int32_t channel)
    {
        for (const AggregateScan& a : scans)
            if (a.kind == kind && a.channel == channel) return &a;
        return nullptr;
    }
    // (null: no such scan was needed)
    static const void* scan_of(const std::vector<AggregateScan>& scans, int32_t kind, int32_t channel)
    {
        const AggregateScan* a = find_scan(scans, kind, channel);
        return a ? a->out : nullptr;
    }

    // The gathers and scans the aggregate functions ask for, each once: per argument channel its NULL flags in sorted order and their
    // count scan (only when the channel has NULLs), its values in sorted order (only for sum / min / max), then one scan per distinct
    // (kind, channel).  Everything lives in aggregates_, laid out here.
    std::vector<AggregateScan> run_aggregate_scans(const int32_t* perm, const int32_t* part_flag, int32_t n, int32_t* error, hipStream_t s)
    {
        struct Channel {
            int32_t channel;
            bool values;
            size_t nulls_at, values_at;
        };
        std::vector<Channel> channels;
        std::vector<AggregateScan> scans;
        std::vector<size_t> scan_at;
        size_t bytes = 0;
        auto take = [&bytes](size_t b) {
            const size_t at = bytes;
            bytes += round_up_256(b);
            return at;
        };
        auto want_scan = [&](int32_t kind, int32_t channel) {
            if (find_scan(scans, kind, channel) != nullptr) return;
            scans.push_back(AggregateScan{kind, channel, nullptr});   // (out: set below, once the buffer stands)
            scan_at.push_back(take((size_t)n * (kind == kWindowScanCount ? 4 : 8)));
        };
        for (const FunctionSpec& f : functions_) {
            if (!is_aggregate(f.function) || f.argument_channel < 0) continue;
            const bool has_nulls = held_.cols[f.argument_channel].has_nulls, values = f.function != PA_WINDOW_COUNT;
            if (!has_nulls && !values) continue;
            auto at = std::find_if(channels.begin(), channels.end(), [&](const Channel& c) { return c.channel == f.argument_channel; });
            if (at == channels.end()) at = channels.insert(at, Channel{f.argument_channel, false, has_nulls ? take((size_t)n) : 0, 0});
            if (values && !at->values) {
                at->values = true;
                at->values_at = take((size_t)n * 8);
            }
            if (has_nulls) want_scan(kWindowScanCount, f.argument_channel);
            if (values) want_scan(scan_kind_of(f.function), f.argument_channel);
        }
        if (scans.empty()) return scans;
        const size_t temp_at = take(window_scan_temp_bytes(n));
        char* base = static_cast<char*>(aggregates_.ensure(bytes));
        for (const Channel& c : channels) {
            const DevColumn h = held_.view(c.channel);
            launch_window_gather(h.type, h.values, h.nulls, perm, n, c.values ? reinterpret_cast<uint64_t*>(base + c.values_at) : nullptr,
                                 h.nulls ? reinterpret_cast<uint8_t*>(base + c.nulls_at) : nullptr, s);
        }
        for (size_t k = 0; k < scans.size(); k++) {
            const Channel& c = *std::find_if(channels.begin(), channels.end(), [&](const Channel& ch) { return ch.channel == scans[k].channel; });
            const int32_t t = types_[c.channel];
            const bool has_nulls = held_.cols[c.channel].has_nulls;
            scans[k].out = base + scan_at[k];
            launch_window_scan((WindowScanKind)scans[k].kind, t == PA_DOUBLE || t == PA_REAL, c.values ? reinterpret_cast<const uint64_t*>(base + c.values_at) : nullptr,
                               has_nulls ? reinterpret_cast<const uint8_t*>(base + c.nulls_at) : nullptr, part_flag, n, base + scan_at[k], error, base + temp_at, s);
        }
        return scans;
    }

    Stream stream_;
    PageStager stager_;
    std::vector<int32_t> types_, output_channels_, order_channels_, orders_;
    std::vector<FunctionSpec> functions_;
    size_t partition_count_ = 0;   // the first of order_channels_ are the partition channels
    std::vector<bool> needed_;
    int32_t output_mem_ = PA_MEM_HOST;
    HeldRows held_;
    RowSorter sorter_;
    DevBuf flags_, starts_, words_, scan_temp_;
    PositionGather gather_;
    DevBuf aggregates_;            // the aggregates' sorted arguments, scanned states and tile states
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> storage_;
    bool finishing_ = false, done_ = false;
};

}  // namespace

pa_operator* make_window(const pa_window_desc* desc) { return new WindowOperator(desc); }
pa_operator* make_framed_window(const pa_framed_window_desc* desc) { return new WindowOperator(desc); }

}  // namespace pa
