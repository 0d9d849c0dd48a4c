// op_distinct.cpp -- MarkDistinctOperator and DistinctLimitOperator on device.
//
// Reference path replaced:
//   LocalExecutionPlanner.visitMarkDistinct / visitDistinctLimit (…/sql/planner/LocalExecutionPlanner.java:1540, :1455)
//   MarkDistinctOperator (…/operator/MarkDistinctOperator.java), MarkDistinctHash (…/operator/MarkDistinctHash.java:52-69)
//   DistinctLimitOperator (…/operator/DistinctLimitOperator.java:175-223)
// both over GroupByHash.getGroupIds: a row is "new" when its group id equals the number of groups seen before it.
//
// Contract (include/presto_amd.h).  mark[i] = true exactly when no earlier row -- of an earlier page, or at a smaller position of this
// page -- has a key not distinct from row i's, over the operator's whole life.  Keys compare by IS NOT DISTINCT FROM: NULL is one
// value per channel, every NaN one value, -0.0 is +0.0, VARCHAR compares bytes, any non-zero BOOLEAN byte is true.
// MarkDistinct: output page = input page + that BOOLEAN column (Page.appendColumn).  DistinctLimit: the marked rows' distinct channels
// (and the hash channel), the first `limit` of them in arrival order.
//
// DistinctHash (distinct_hash.hpp) is the table both share: per page canonicalise -> insert -> mark -> scan -> publish.  The descriptor
// checks, and MarkDistinct's output page with the retained input page behind it (PassThroughOutput), are keyed_operator.hpp's.
#include "keyed_operator.hpp"

namespace pa {
namespace {

// what both descriptors share, checked before the device is asked for: a shape the device path does not take is reported as such
// with or without a GPU
void check_distinct_desc(int32_t channels, const int32_t* types, int32_t distinct_count, const int32_t* distinct_channels, int32_t hash_channel,
                         int32_t expected, int32_t output_mem)
{
    PA_REQUIRE(types != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    check_input_channels(channels);
    PA_REQUIRE(distinct_count > 0 && distinct_channels != nullptr, PA_ERR_INVALID_ARGUMENT, "no distinct channels");
    PA_REQUIRE(distinct_count <= kMaxJoinChannels, PA_ERR_NOT_SUPPORTED, "more distinct channels than the device path takes");
    check_key_channels(distinct_channels, distinct_count, channels, types, "distinct");
    check_hash_channel(hash_channel, channels, types);
    PA_REQUIRE(expected >= 0, PA_ERR_INVALID_ARGUMENT, "expected_distinct is negative");
    check_output_mem(output_mem);
}
void* checked_stream(const pa_mark_distinct_desc* d)
{
    PA_REQUIRE(d != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    check_distinct_desc(d->input_channel_count, d->input_types, d->distinct_channel_count, d->distinct_channels, d->hash_channel, d->expected_distinct,
                        d->output_mem);
    return d->stream;
}
void* checked_stream(const pa_distinct_limit_desc* d)
{
    PA_REQUIRE(d != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    check_distinct_desc(d->input_channel_count, d->input_types, d->distinct_channel_count, d->distinct_channels, d->hash_channel, d->expected_distinct,
                        d->output_mem);
    PA_REQUIRE(d->limit >= 0, PA_ERR_INVALID_ARGUMENT, "limit is negative");
    return d->stream;
}

// what the two operators share: descriptor fields, staging of the key channels, the table
class DistinctBase : public pa_operator {
public:
    template <class Desc>
    explicit DistinctBase(const Desc* d) : stream_(checked_stream(d))
    {
        types_.assign(d->input_types, d->input_types + d->input_channel_count);
        distinct_channels_.assign(d->distinct_channels, d->distinct_channels + d->distinct_channel_count);
        hash_channel_ = d->hash_channel;
        output_mem_ = d->output_mem;
        hash_ = make_distinct_hash(types_, distinct_channels_, d->expected_distinct, stream_.get());
    }
    ~DistinctBase() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }
    void stats(int64_t* distinct_count, int64_t* table_capacity)
    {
        if (distinct_count) *distinct_count = hash_->settle(stream_.get());
        if (table_capacity) *table_capacity = hash_->capacity();
    }

protected:
    const char* add_keys(const DevPage& in, int32_t n, uint8_t* mark, int32_t* out_positions, int64_t limit)
    {
        return hash_->add_page(KeyColumns(in, distinct_channels_).cols, n, mark, out_positions, limit, timer, stream_.get());
    }
    Stream stream_;
    PageStager stager_;
    std::unique_ptr<DistinctHash> hash_;
    std::vector<int32_t> types_, distinct_channels_;
    int32_t hash_channel_ = -1, output_mem_ = PA_MEM_HOST;
};

class MarkDistinctOperator : public DistinctBase {
public:
    explicit MarkDistinctOperator(const pa_mark_distinct_desc* d) : DistinctBase(d)
    {
        pass_.init(types_.size(), all_channels(types_.size()), distinct_channels_, output_mem_);
    }
    ~MarkDistinctOperator() override
    {
        (void)hipStreamSynchronize(stream_.get());
        pass_.release(stream_.get());
    }
    // the output page may be the input page's own blocks: a retained input page is let go once its output page is
    bool takes_retained() override { return true; }

    bool needs_input() override
    {
        if (!pending_) pass_.release(stream_.get());
        return !finishing_ && !pending_;
    }

    void add_input(const pa_page* page) override
    {
        pass_.release(stream_.get());
        pass_.hold(page);
        PA_REQUIRE(!finishing_ && !pending_, PA_ERR_ILLEGAL_STATE, "Operator does not need input");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int32_t n = page->position_count;
        if (n <= 0) return;
        // Page.appendColumn: the input blocks as they are where they can stay (their encodings included), the mark behind them
        const DevPage& in = pass_.stage(stager_, page, true, stream_.get());
        uint8_t* mark = static_cast<uint8_t*>(mark_.ensure(((size_t)n + 3) & ~(size_t)3));
        timer.set_name(add_keys(in, n, mark, nullptr, 0));
        n_ = n;
        pending_ = true;
    }

    bool get_output(pa_page* out) override
    {
        if (!pending_) {
            pass_.release(stream_.get());
            return false;
        }
        pending_ = false;
        pass_.publish(n_, PA_BOOLEAN, mark_.ptr(), nullptr, stream_.get(), out);
        return true;
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finishing_ && !pending_; }
    void close() override
    {
        (void)hipStreamSynchronize(stream_.get());
        pass_.release(stream_.get());
    }
    int64_t memory_bytes() override { return hash_->memory_bytes() + (int64_t)(stager_.bytes() + mark_.capacity()); }

private:
    PassThroughOutput pass_;
    int32_t n_ = 0;
    DevBuf mark_;
    bool pending_ = false, finishing_ = false;
};

class DistinctLimitOperator : public DistinctBase {
public:
    explicit DistinctLimitOperator(const pa_distinct_limit_desc* d) : DistinctBase(d), remaining_(d->limit)
    {
        // output: the distinct channels in descriptor order, then the hash channel (DistinctLimitOperator.java:76-79)
        output_channels_ = distinct_channels_;
        if (hash_channel_ >= 0) output_channels_.push_back(hash_channel_);
        needed_.assign(types_.size(), false);
        for (int32_t c : output_channels_) needed_[c] = true;
    }

    bool needs_input() override { return !finishing_ && remaining_ > 0 && !pending_; }

    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(needs_input(), PA_ERR_ILLEGAL_STATE, "Operator does not need input");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int32_t n = page->position_count;
        if (n <= 0) return;
        hipStream_t s = stream_.get();
        const DevPage in = stager_.stage(page, &needed_, s);
        uint8_t* mark = static_cast<uint8_t*>(mark_.ensure(((size_t)n + 3) & ~(size_t)3));
        const int64_t cap = std::min<int64_t>(n, remaining_);
        int32_t* positions = static_cast<int32_t*>(positions_.ensure((size_t)cap * 4));
        const int64_t before = hash_->settle(s);
        timer.set_name(add_keys(in, n, mark, positions, cap));
        // the page's new keys: the operator's state machine turns on it (DistinctLimitOperator.java:189-203)
        const int64_t k = std::min<int64_t>(hash_->settle(s) - before, remaining_);
        if (k == 0) return;
        remaining_ -= k;
        out_cols_.resize(output_channels_.size());
        // (no 2 GiB message: the first rows of their keys, each once, of ONE staged block -- under 2 GiB, PageStager::stage)
        for (size_t c = 0; c < output_channels_.size(); c++) gather_.copy_positions(in.cols[output_channels_[c]], positions, (int32_t)k, out_cols_[c], s);
        n_ = (int32_t)k;
        pending_ = true;
        if (page->mem != PA_MEM_DEVICE || output_mem_ != PA_MEM_DEVICE) PA_HIP(hipStreamSynchronize(s));
    }

    bool get_output(pa_page* out) override
    {
        if (!pending_) return false;
        pending_ = false;
        publish_output(out_cols_, n_, output_mem_, stream_.get(), out, storage_);
        return true;
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return !pending_ && (finishing_ || remaining_ == 0); }
    void close() override { (void)hipStreamSynchronize(stream_.get()); }
    int64_t memory_bytes() override
    {
        size_t b = stager_.bytes() + mark_.capacity() + positions_.capacity() + gather_.bytes();
        for (const OutColumn& o : out_cols_) b += o.values.capacity() + o.offsets.capacity() + o.nulls.capacity();
        return hash_->memory_bytes() + (int64_t)b;
    }

private:
    std::vector<int32_t> output_channels_;
    std::vector<bool> needed_;
    int64_t remaining_ = 0;
    int32_t n_ = 0;
    DevBuf mark_, positions_;
    PositionGather gather_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> storage_;
    bool pending_ = false, finishing_ = false;
};

}  // namespace

pa_operator* make_mark_distinct(const pa_mark_distinct_desc* desc) { return new MarkDistinctOperator(desc); }
pa_operator* make_distinct_limit(const pa_distinct_limit_desc* desc) { return new DistinctLimitOperator(desc); }
void distinct_stats(pa_operator* op, int64_t* distinct_count, int64_t* table_capacity)
{
    DistinctBase* d = dynamic_cast<DistinctBase*>(op);
    PA_REQUIRE(d != nullptr, PA_ERR_INVALID_ARGUMENT, "not a MarkDistinct / DistinctLimit operator");
    d->stats(distinct_count, table_capacity);
}

}  // namespace pa
