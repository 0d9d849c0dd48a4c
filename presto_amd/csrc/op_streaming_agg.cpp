// op_streaming_agg.cpp -- StreamingAggregationOperator on device: the aggregation over input that arrives grouped.
//
// Reference path replaced:
//   LocalExecutionPlanner.visitAggregation, the streamable branch (pre-grouped symbols = all grouping keys, step SINGLE)
//   StreamingAggregationOperator (…/operator/StreamingAggregationOperator.java:171-367): addInput / aggregateBatch / evaluateAndFlushGroup
// -- the last operator of every decorrelated scalar subquery: AssignUniqueId -> LookupJoin (probe outer, which keeps probe order) ->
// this, grouped by the unique id.
//
// Contract (include/presto_amd.h).  One output row per run of rows that are NOT DISTINCT on the group channels, in input order: the
// group columns of the run's first row, then the aggregates.  A run is emitted once a row of another run has been seen, or at finish.
//
// No table: per page flags -> scan -> run starts -> the segmented reduction of all aggregates (streaming_agg_kernels.hpp), then ONE
// read-back of {runs closed in the page, error word}, then the group columns of the closed runs through PositionGather.  What a page
// leaves open lives in the operator's own HBM: the first-row key as one-row columns (VARCHAR bytes included) and one 16-byte state per
// aggregate, double-buffered so that no launch reads what it writes.  The aggregate columns are sized for a run per row before the
// count is known -- that is the price of the single read-back.
#include "keyed_operator.hpp"
#include "streaming_agg_kernels.hpp"

namespace pa {
namespace {

bool known_type(int32_t t)
{
    switch (t) {
        case PA_BIGINT:
        case PA_INTEGER:
        case PA_DATE:
        case PA_DOUBLE:
        case PA_REAL:
        case PA_BOOLEAN:
        case PA_VARCHAR:
        case PA_DECIMAL:
        case PA_LONG_DECIMAL:
        case PA_ROW: return true;
        default: return false;
    }
}

// every invalid argument of the descriptor first, then what the device path refuses; both before the device is asked for
void* checked_stream(const pa_streaming_aggregation_desc* d)
{
    PA_REQUIRE(d != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    PA_REQUIRE(d->input_channel_count > 0 && d->input_types != nullptr, PA_ERR_INVALID_ARGUMENT, "no input channels");
    PA_REQUIRE(d->group_by_count >= 1 && d->group_by_count <= kStreamAggMaxKeys && d->group_by_channels != nullptr, PA_ERR_INVALID_ARGUMENT,
               "1..8 group channels");
    PA_REQUIRE(d->aggregate_count >= 0 && d->aggregate_count <= kStreamAggMaxAggregates && (d->aggregate_count == 0 || d->aggregates != nullptr),
               PA_ERR_INVALID_ARGUMENT, "0..16 aggregates");
    PA_REQUIRE(d->step == PA_STEP_SINGLE || d->step == PA_STEP_PARTIAL || d->step == PA_STEP_FINAL, PA_ERR_INVALID_ARGUMENT, "unknown step");
    check_output_mem(d->output_mem);
    const int32_t channels = d->input_channel_count;
    for (int32_t c = 0; c < channels; c++) PA_REQUIRE(known_type(d->input_types[c]), PA_ERR_INVALID_ARGUMENT, "unknown input type");
    check_channels(d->group_by_channels, d->group_by_count, channels, "group");
    for (int32_t i = 0; i < d->aggregate_count; i++) {
        const pa_aggregate& a = d->aggregates[i];
        PA_REQUIRE(a.fn >= PA_AGG_COUNT_STAR && a.fn <= PA_AGG_MAX, PA_ERR_INVALID_ARGUMENT, "unknown aggregate function");
        PA_REQUIRE(a.mask_channel >= -1 && a.mask_channel < channels, PA_ERR_INVALID_ARGUMENT, "mask channel out of range");
        PA_REQUIRE(a.mask_channel < 0 || d->input_types[a.mask_channel] == PA_BOOLEAN, PA_ERR_INVALID_ARGUMENT, "mask channel must be BOOLEAN");
        if (a.fn == PA_AGG_COUNT_STAR) continue;
        PA_REQUIRE(a.input_channel >= 0 && a.input_channel < channels, PA_ERR_INVALID_ARGUMENT, "aggregate input channel out of range");
        const int32_t t = d->input_types[a.input_channel];
        PA_REQUIRE(a.input_type == t, PA_ERR_INVALID_ARGUMENT, "aggregate input_type differs from the channel's type");
        if (a.fn == PA_AGG_SUM || a.fn == PA_AGG_AVG)
            PA_REQUIRE(t != PA_VARCHAR && t != PA_BOOLEAN && t != PA_DATE && t != PA_ROW, PA_ERR_INVALID_ARGUMENT, "sum / avg over a type without one");
    }
    // ---- refusals
    PA_REQUIRE(d->step == PA_STEP_SINGLE, PA_ERR_NOT_SUPPORTED, "streaming aggregation: only step SINGLE on the device");
    check_input_channels(channels);
    for (int32_t i = 0; i < d->group_by_count; i++) check_key_type(d->input_types[d->group_by_channels[i]], "group");
    for (int32_t i = 0; i < d->aggregate_count; i++) {
        const pa_aggregate& a = d->aggregates[i];
        if (a.fn == PA_AGG_COUNT_STAR) continue;
        const int32_t t = d->input_types[a.input_channel];
        if (a.fn == PA_AGG_COUNT) PA_REQUIRE(t != PA_ROW, PA_ERR_NOT_SUPPORTED, "count over PA_ROW");
        if (a.fn == PA_AGG_SUM || a.fn == PA_AGG_AVG)
            PA_REQUIRE(t != PA_DECIMAL && t != PA_LONG_DECIMAL, PA_ERR_NOT_SUPPORTED, "streaming aggregation: sum / avg over DECIMAL");
        if (a.fn == PA_AGG_MIN || a.fn == PA_AGG_MAX)
            PA_REQUIRE(t != PA_VARCHAR && t != PA_LONG_DECIMAL && t != PA_ROW, PA_ERR_NOT_SUPPORTED, "streaming aggregation: min / max over this type");
    }
    return d->stream;
}

// the type of an aggregate's result column (tests/agg_model.result_type)
int32_t result_type(const pa_aggregate& a)
{
    if (a.fn == PA_AGG_COUNT_STAR || a.fn == PA_AGG_COUNT) return PA_BIGINT;
    if (a.fn == PA_AGG_AVG) return a.input_type == PA_REAL ? PA_REAL : PA_DOUBLE;
    return a.input_type;
}

DevColumn column_of(const OutColumn& o)
{
    DevColumn c;
    c.type = o.type;
    c.varwidth = o.varwidth;
    c.values = o.values.ptr();
    c.offsets = static_cast<const int32_t*>(o.offsets.ptr());
    c.nulls = o.has_nulls ? static_cast<const uint8_t*>(o.nulls.ptr()) : nullptr;
    return c;
}

class StreamingAggregationOperator : public pa_operator {
public:
    explicit StreamingAggregationOperator(const pa_streaming_aggregation_desc* d) : stream_(checked_stream(d)), output_mem_(d->output_mem)
    {
        types_.assign(d->input_types, d->input_types + d->input_channel_count);
        group_channels_.assign(d->group_by_channels, d->group_by_channels + d->group_by_count);
        aggregates_.assign(d->aggregates, d->aggregates + d->aggregate_count);
        needed_.assign(types_.size(), false);
        for (int32_t c : group_channels_) needed_[c] = true;
        for (const pa_aggregate& a : aggregates_) {
            if (a.fn != PA_AGG_COUNT_STAR) needed_[a.input_channel] = true;
            if (a.mask_channel >= 0) needed_[a.mask_channel] = true;
        }
        const size_t nk = group_channels_.size(), na = aggregates_.size();
        carry_key_.resize(nk);
        carry_bytes_.assign(nk, 0);
        out_cols_.resize(nk + na);
        for (size_t i = 0; i < na; i++) {
            OutColumn& o = out_cols_[nk + i];
            o.type = result_type(aggregates_[i]);
            o.has_nulls = aggregates_[i].fn != PA_AGG_COUNT_STAR && aggregates_[i].fn != PA_AGG_COUNT;
        }
        hipStream_t s = stream_.get();
        PA_HIP(hipMemsetAsync(carry_state_[0].ensure(kStreamAggMaxAggregates * sizeof(StreamAggState)), 0, kStreamAggMaxAggregates * sizeof(StreamAggState), s));
        PA_HIP(hipMemsetAsync(carry_state_[1].ensure(kStreamAggMaxAggregates * sizeof(StreamAggState)), 0, kStreamAggMaxAggregates * sizeof(StreamAggState), s));
        info_.ensure(64);
    }
    ~StreamingAggregationOperator() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }

    bool needs_input() override { return !finishing_ && !pending_ && !failed_; }

    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(!failed_, fail_status_, fail_message_);
        PA_REQUIRE(!finishing_ && !pending_, PA_ERR_ILLEGAL_STATE, "Operator does not need input");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int32_t n = page->position_count;
        if (n <= 0) return;   // an empty page neither closes nor opens a run
        hipStream_t s = stream_.get();
        const DevPage in = stager_.stage(page, &needed_, s);
        const size_t nk = group_channels_.size(), na = aggregates_.size();

        int32_t* flags = static_cast<int32_t*>(flags_.ensure((size_t)n * 4));
        int32_t* idx = static_cast<int32_t*>(idx_.ensure((size_t)n * 4));
        int32_t* start = static_cast<int32_t*>(start_.ensure(((size_t)n + 1) * 4));
        int32_t* info = info_.as<int32_t>();   // [0] the runs closed in the page (the scan's total), [1] the error word
        PA_HIP(hipMemsetAsync(info, 0, 8, s));

        StreamAggFlagArgs fa{};
        fa.count = (int32_t)nk;
        fa.n = n;
        fa.open = open_ ? 1 : 0;
        fa.flags = flags;
        for (size_t c = 0; c < nk; c++) {
            const DevColumn& col = in.cols[group_channels_[c]];
            StreamAggKey& k = fa.k[c];
            k.type = col.type;
            k.values = col.values;
            k.offsets = col.offsets;
            k.nulls = col.nulls;
            if (open_) {
                const DevColumn carried = column_of(carry_key_[c]);
                k.carry_values = carried.values;
                k.carry_offsets = carried.offsets;
                k.carry_nulls = carried.nulls;
            }
        }
        timer.set_name("k_stream_agg_apply");
        launch_stream_agg_flags(fa, s);
        launch_exclusive_scan_i32(flags, idx, n, info, scan_temp_.ensure(scan_temp_bytes(n)), s);
        launch_stream_agg_starts(flags, idx, n, start, s);
        if (na > 0) {
            StreamAggArgs ra = reduce_args(&in, n);
            ra.flags = flags;
            ra.idx = idx;
            ra.closed = info;
            ra.error = info + 1;
            timer.begin(s);
            launch_stream_agg_reduce(ra, s);
            timer.end(s);
        }

        int32_t h_info[2] = {0, 0};
        read_back(h_info, info, 8, s);   // the one read-back of the page
        const int32_t closed = h_info[0], error = h_info[1];
        PA_REQUIRE(closed >= 0 && closed <= n, PA_ERR_DEVICE, "streaming aggregation: closed runs out of range");
        if (na > 0) cur_ ^= 1;           // the states at row n - 1 are the carry now
        // a prefix that left int64 fails the call that would hand out its run: now for the runs that closed, later for the run left open
        const bool carried_closes = open_ && closed >= 1;
        if ((error & kStreamAggErrorClosed) != 0 || (carried_closes && open_overflowed_)) fail();
        open_overflowed_ = (closed >= 1 ? false : open_overflowed_) || (error & kStreamAggErrorOpen) != 0;

        if (closed >= 1) {
            for (size_t c = 0; c < nk; c++) gather_key(in.cols[group_channels_[c]], c, start, closed, s);
            n_ = closed;
            pending_ = true;
        }
        // the first row of the run the page leaves open: row start[closed], unless the carried run goes on
        if (!open_ || closed >= 1) {
            // (no 2 GiB message: ONE row of one staged block -- under 2 GiB, PageStager::stage)
            for (size_t c = 0; c < nk; c++) carry_bytes_[c] = gather_.copy_positions(in.cols[group_channels_[c]], start + closed, 1, carry_key_[c], s);
        }
        open_ = true;
        if (page->mem != PA_MEM_DEVICE || output_mem_ != PA_MEM_DEVICE) PA_HIP(hipStreamSynchronize(s));
    }

    bool get_output(pa_page* out) override
    {
        if (failed_) return false;
        if (!pending_ && finishing_ && open_) flush_open_run();   // behind the last page of closed runs: the run finish closes
        if (!pending_) return false;
        pending_ = false;
        publish_output(out_cols_, n_, output_mem_, stream_.get(), out, storage_);
        return true;
    }

    void finish() override { finishing_ = true; }
    // (no input at all: no run is open, no output)
    bool is_finished() override { return failed_ || (finishing_ && !pending_ && !open_); }
    void close() override { (void)hipStreamSynchronize(stream_.get()); }

private:
    // the run that finish closes, as an output page of one row: its key from the carry, its aggregates from the carried states
    void flush_open_run()
    {
        hipStream_t s = stream_.get();
        const size_t nk = group_channels_.size(), na = aggregates_.size();
        if (na > 0) {
            int32_t* info = info_.as<int32_t>();
            PA_HIP(hipMemsetAsync(info, 0, 8, s));
            StreamAggArgs ra = reduce_args(nullptr, 1);
            ra.error = info + 1;
            launch_stream_agg_finish(ra, s);
            int32_t h_info[2] = {0, 0};
            read_back(h_info, info, 8, s);
            if ((h_info[1] & kStreamAggErrorClosed) != 0 || open_overflowed_) fail();
        }
        for (size_t c = 0; c < nk; c++) view_column(out_cols_[c], column_of(carry_key_[c]));
        open_ = false;
        n_ = 1;
        pending_ = true;
    }

public:
    int64_t memory_bytes() override
    {
        size_t b = stager_.bytes() + flags_.capacity() + idx_.capacity() + start_.capacity() + scan_temp_.capacity() + tile_acc_.capacity() + tile_front_.capacity() +
                   gather_.bytes() + carry_state_[0].capacity() + carry_state_[1].capacity() + info_.capacity();
        for (const OutColumn& o : out_cols_) b += o.values.capacity() + o.offsets.capacity() + o.nulls.capacity();
        for (const OutColumn& o : carry_key_) b += o.values.capacity() + o.offsets.capacity() + o.nulls.capacity();
        b += rest_.values.capacity() + rest_.offsets.capacity() + rest_.nulls.capacity();
        return (int64_t)b;
    }

private:
    static constexpr const char* kOutOfRange = "bigint addition overflow in sum: a running sum of a group left the range of its type";

    static constexpr const char* kKeyColumnTooLarge =
        "the group keys of the runs a page closes, the carried run's among them, hold more than 2 GB of VARCHAR bytes in one output column";

    // (the operator is done for: its carry has moved on past rows that no page of output holds)
    [[noreturn]] void fail(int32_t status = PA_ERR_NUMERIC_VALUE_OUT_OF_RANGE, const char* message = kOutOfRange)
    {
        failed_ = true;
        pending_ = false;
        fail_status_ = status;
        fail_message_ = message;
        throw Error(status, message);
    }

    // the arguments of the reduction over page `in` (null: only what the finish launch reads), its output columns sized for n runs
    StreamAggArgs reduce_args(const DevPage* in, int32_t n)
    {
        const size_t nk = group_channels_.size(), na = aggregates_.size();
        StreamAggArgs ra{};
        ra.n = n;
        ra.tiles = stream_agg_tiles(n);
        ra.count = (int32_t)na;
        ra.open = open_ ? 1 : 0;
        ra.carry_in = carry_state_[cur_].as<StreamAggState>();
        ra.carry_out = carry_state_[cur_ ^ 1].as<StreamAggState>();
        if (in != nullptr) {
            ra.tile_acc = static_cast<StreamAggState*>(tile_acc_.ensure(na * (size_t)ra.tiles * sizeof(StreamAggState)));
            ra.tile_front = static_cast<StreamAggState*>(tile_front_.ensure(na * (size_t)ra.tiles * sizeof(StreamAggState)));
        }
        for (size_t i = 0; i < na; i++) {
            const pa_aggregate& a = aggregates_[i];
            StreamAggFn& f = ra.f[i];
            f.fn = a.fn;
            f.in_type = a.fn == PA_AGG_COUNT_STAR ? PA_BIGINT : a.input_type;
            const bool floating = f.in_type == PA_DOUBLE || f.in_type == PA_REAL;
            switch (a.fn) {
                case PA_AGG_COUNT_STAR:
                case PA_AGG_COUNT: f.kind = kStreamAggCount; break;
                case PA_AGG_SUM: f.kind = floating ? kStreamAggSumDouble : kStreamAggSumInt; break;
                case PA_AGG_AVG: f.kind = kStreamAggSumDouble; break;
                case PA_AGG_MIN: f.kind = kStreamAggMin; break;
                default: f.kind = kStreamAggMax; break;
            }
            f.cmp = f.in_type == PA_DOUBLE ? kStreamAggCmpDouble : f.in_type == PA_REAL ? kStreamAggCmpFloat : kStreamAggCmpInt;
            if (in != nullptr) {
                if (a.fn != PA_AGG_COUNT_STAR) {
                    f.values = in->cols[a.input_channel].values;
                    f.nulls = in->cols[a.input_channel].nulls;
                }
                if (a.mask_channel >= 0) {
                    f.mask_values = static_cast<const uint8_t*>(in->cols[a.mask_channel].values);
                    f.mask_nulls = in->cols[a.mask_channel].nulls;
                }
            }
            OutColumn& o = out_cols_[nk + i];
            o.is_view = false;
            o.host_ready = false;
            f.out = o.values.ensure((size_t)n * type_width(o.type));
            f.out_nulls = o.has_nulls ? static_cast<uint8_t*>(o.nulls.ensure((size_t)n)) : nullptr;
        }
        return ra;
    }

    // Group channel c of the k runs that closed: the rows start[0 .. k) of the page through PositionGather -- except that with a run
    // carried in, run 0's first row is in the carry: a fixed-width column gathers the placeholder start[0] = 0 and has its row 0 replaced,
    // a VARCHAR column is the carried string with the gather of the other k - 1 runs behind it.
    void gather_key(const DevColumn& src, size_t c, const int32_t* start, int32_t k, hipStream_t s)
    {
        OutColumn& o = out_cols_[c];
        if (!open_) {
            gather_.copy_positions(src, start, k, o, s);   // (no 2 GiB message: run start rows, each once, of ONE staged block)
            return;
        }
        const OutColumn& carried = carry_key_[c];
        const void* carried_null = carried.has_nulls ? carried.nulls.ptr() : nullptr;
        if (!src.varwidth) {
            gather_.copy_positions(src, start, k, o, s);
            const int w = type_width(src.type);
            PA_HIP(hipMemcpyAsync(o.values.ptr(), carried.values.ptr(), (size_t)w, hipMemcpyDeviceToDevice, s));
            if (!o.has_nulls) {
                PA_HIP(hipMemsetAsync(o.nulls.ensure((size_t)k), 0, (size_t)k, s));
                o.has_nulls = true;
            }
            if (carried_null) PA_HIP(hipMemcpyAsync(o.nulls.ptr(), carried_null, 1, hipMemcpyDeviceToDevice, s));
            else PA_HIP(hipMemsetAsync(o.nulls.ptr(), 0, 1, s));
            return;
        }
        const int32_t head = carry_bytes_[c];
        int32_t rest = 0;
        // (no 2 GiB message for `rest`: run start rows, each once, of ONE staged block -- under 2 GiB, PageStager::stage.  But the column is
        // that AND the carried key, which came with an earlier block: their sum is checked here, before the buffer is sized by it)
        if (k > 1) rest = gather_.copy_positions(src, start + 1, k - 1, rest_, s);
        if ((int64_t)head + rest > INT32_MAX) fail(PA_ERR_INSUFFICIENT_RESOURCES, kKeyColumnTooLarge);
        o.type = src.type;
        o.varwidth = true;
        o.has_nulls = true;
        o.is_view = false;
        o.host_ready = false;
        uint8_t* bytes = static_cast<uint8_t*>(o.values.ensure((size_t)std::max(head + rest, 1)));
        int32_t* offsets = static_cast<int32_t*>(o.offsets.ensure(((size_t)k + 1) * 4));
        uint8_t* nulls = static_cast<uint8_t*>(o.nulls.ensure((size_t)k));
        head_offsets_[2 * c] = 0;   // (a buffer per channel: the copy may run after this call returns)
        head_offsets_[2 * c + 1] = head;
        PA_HIP(hipMemcpyAsync(offsets, &head_offsets_[2 * c], 8, hipMemcpyHostToDevice, s));
        if (head > 0) PA_HIP(hipMemcpyAsync(bytes, carried.values.ptr(), (size_t)head, hipMemcpyDeviceToDevice, s));
        if (carried_null) PA_HIP(hipMemcpyAsync(nulls, carried_null, 1, hipMemcpyDeviceToDevice, s));
        else PA_HIP(hipMemsetAsync(nulls, 0, 1, s));
        if (k > 1) {
            launch_offsets_append(static_cast<const int32_t*>(rest_.offsets.ptr()), k - 1, head, offsets + 1, false, s);
            if (rest > 0) PA_HIP(hipMemcpyAsync(bytes + head, rest_.values.ptr(), (size_t)rest, hipMemcpyDeviceToDevice, s));
            if (rest_.has_nulls) PA_HIP(hipMemcpyAsync(nulls + 1, rest_.nulls.ptr(), (size_t)(k - 1), hipMemcpyDeviceToDevice, s));
            else PA_HIP(hipMemsetAsync(nulls + 1, 0, (size_t)(k - 1), s));
        }
    }

    Stream stream_;
    int32_t output_mem_ = PA_MEM_HOST;
    std::vector<int32_t> types_, group_channels_;
    std::vector<pa_aggregate> aggregates_;
    std::vector<bool> needed_;
    PageStager stager_;
    PositionGather gather_;
    DevBuf flags_, idx_, start_, scan_temp_, tile_acc_, tile_front_, info_;
    // the carry: the open run's first-row key per group channel as one-row columns (carry_bytes_: a VARCHAR key's length), and its state per
    // aggregate in carry_state_[cur_]
    std::vector<OutColumn> carry_key_;
    std::vector<int32_t> carry_bytes_;
    DevBuf carry_state_[2];
    int cur_ = 0;
    bool open_ = false;              // a run is open: some row has been seen and finish has not
    bool open_overflowed_ = false;   // a prefix of the open run's BIGINT sum left int64: the call that closes the run fails
    OutColumn rest_;                 // a VARCHAR key column's runs 1 .. k - 1 on their way behind the carried string
    int32_t head_offsets_[2 * kStreamAggMaxKeys] = {};
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> storage_;
    int32_t n_ = 0;
    bool pending_ = false, finishing_ = false, failed_ = false;
    int32_t fail_status_ = PA_ERR_NUMERIC_VALUE_OUT_OF_RANGE;   // what a failed operator answers every later call with
    const char* fail_message_ = kOutOfRange;
};

}  // namespace

pa_operator* make_streaming_aggregation(const pa_streaming_aggregation_desc* desc) { return new StreamingAggregationOperator(desc); }

}  // namespace pa
