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
// DistinctHash (distinct_hash.hpp) is the table both share: per page canonicalise -> insert -> mark -> scan -> publish.
#include <deque>

#include "distinct_hash.hpp"
#include "operator.hpp"

namespace pa {
namespace {

// what both descriptors share, checked before the device is asked for: a shape the device path does not take is reported as such
// with or without a GPU
void check_distinct_desc(int32_t channels, const int32_t* types, int32_t distinct_count, const int32_t* distinct_channels, int32_t hash_channel,
                         int32_t expected, int32_t output_mem)
{
    PA_REQUIRE(types != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    PA_REQUIRE(channels > 0 && channels <= 64, PA_ERR_NOT_SUPPORTED, "1..64 input channels");
    PA_REQUIRE(distinct_count > 0 && distinct_channels != nullptr, PA_ERR_INVALID_ARGUMENT, "no distinct channels");
    PA_REQUIRE(distinct_count <= kMaxJoinChannels, PA_ERR_NOT_SUPPORTED, "more distinct channels than the device path takes");
    for (int32_t i = 0; i < distinct_count; i++) {
        const int32_t c = distinct_channels[i];
        PA_REQUIRE(c >= 0 && c < channels, PA_ERR_INVALID_ARGUMENT, "distinct channel out of range");
        switch (types[c]) {
            case PA_BIGINT:
            case PA_INTEGER:
            case PA_DATE:
            case PA_DOUBLE:
            case PA_REAL:
            case PA_BOOLEAN:
            case PA_VARCHAR:
            case PA_DECIMAL: break;
            case PA_LONG_DECIMAL:
            case PA_ROW: throw Error(PA_ERR_NOT_SUPPORTED, "distinct key type not supported on the device");
            default: throw Error(PA_ERR_INVALID_ARGUMENT, "unknown distinct key type");
        }
    }
    PA_REQUIRE(hash_channel >= -1 && hash_channel < channels, PA_ERR_INVALID_ARGUMENT, "hash channel out of range");
    PA_REQUIRE(hash_channel < 0 || types[hash_channel] == PA_BIGINT, PA_ERR_INVALID_ARGUMENT, "hash channel must be BIGINT");
    PA_REQUIRE(expected >= 0, PA_ERR_INVALID_ARGUMENT, "expected_distinct is negative");
    PA_REQUIRE(output_mem == PA_MEM_HOST || output_mem == PA_MEM_DEVICE, PA_ERR_INVALID_ARGUMENT, "unknown output_mem");
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
        std::vector<int32_t> key_types;
        for (int32_t c : distinct_channels_) key_types.push_back(types_[c]);
        hash_.reset(new DistinctHash(key_types, d->expected_distinct, stream_.get()));
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
        const DevColumn* cols[kMaxJoinChannels];
        for (size_t i = 0; i < distinct_channels_.size(); i++) cols[i] = &in.cols[distinct_channels_[i]];
        return hash_->add_page(cols, n, mark, out_positions, limit, timer, stream_.get());
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
        key_only_.assign(types_.size(), false);
        for (int32_t c : distinct_channels_) key_only_[c] = true;
    }
    ~MarkDistinctOperator() override
    {
        (void)hipStreamSynchronize(stream_.get());
        release_held();
    }
    // the output page may be the input page's own blocks: a retained input page is let go once its output page is
    bool takes_retained() override { return true; }

    bool needs_input() override
    {
        if (!pending_) release_held();
        return !finishing_ && !pending_;
    }

    void add_input(const pa_page* page) override
    {
        release_held();
        if (page != nullptr && (page->flags & PA_PAGE_RETAINED) != 0 && page->release != nullptr) held_ = {page->release, page->release_ctx};
        PA_REQUIRE(!finishing_ && !pending_, PA_ERR_ILLEGAL_STATE, "Operator does not need input");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int32_t n = page->position_count;
        if (n <= 0) return;
        hipStream_t s = stream_.get();
        zero_copy_ = page->mem == PA_MEM_DEVICE && output_mem_ == PA_MEM_DEVICE;
        in_ = stager_.stage(page, zero_copy_ ? &key_only_ : nullptr, s);
        if (zero_copy_) {
            // Page.appendColumn: the input blocks as they are (their encodings included), the mark behind them
            dict_copies_.clear();
            storage_.resize(types_.size() + 1);
            for (size_t c = 0; c < types_.size(); c++) storage_[c] = copy_column(page->columns[c]);
        }
        uint8_t* mark = static_cast<uint8_t*>(mark_.ensure(((size_t)n + 3) & ~(size_t)3));
        timer.set_name(add_keys(in_, n, mark, nullptr, 0));
        n_ = n;
        pending_ = true;
    }

    bool get_output(pa_page* out) override
    {
        if (!pending_) {
            release_held();
            return false;
        }
        pending_ = false;
        const size_t nc = types_.size();
        if (zero_copy_) {
            pa_column& m = storage_[nc];
            memset(&m, 0, sizeof m);
            m.type = PA_BOOLEAN;
            m.encoding = PA_FLAT;
            m.values = mark_.ptr();
            out->position_count = n_;
            out->channel_count = (int32_t)nc + 1;
            out->columns = storage_.data();
            out->mem = PA_MEM_DEVICE;
            out->flags = 0;
            out->release = nullptr;
            out->release_ctx = nullptr;
            return true;
        }
        out_cols_.resize(nc + 1);
        for (size_t c = 0; c <= nc; c++) {
            OutColumn& o = out_cols_[c];
            o.is_view = true;
            o.host_ready = false;
            if (c < nc) {
                const DevColumn& src = in_.cols[c];
                o.type = src.type;
                o.varwidth = src.varwidth;
                o.has_nulls = src.nulls != nullptr;
                o.view_values = src.values;
                o.view_offsets = src.offsets;
                o.view_nulls = src.nulls;
            }
            else {
                o.type = PA_BOOLEAN;
                o.varwidth = false;
                o.has_nulls = false;
                o.view_values = mark_.ptr();
                o.view_offsets = nullptr;
                o.view_nulls = nullptr;
            }
        }
        publish_output(out_cols_, n_, output_mem_, stream_.get(), out, storage_);
        return true;
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finishing_ && !pending_; }
    void close() override
    {
        (void)hipStreamSynchronize(stream_.get());
        release_held();
    }
    int64_t memory_bytes() override { return hash_->memory_bytes() + (int64_t)(stager_.bytes() + mark_.capacity()); }

private:
    // a block of the input page, its dictionary (DICTIONARY / RLE / ROW_FIELDS) copied: the caller's pa_column structs are its own
    // again when add_input returns
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
    void release_held()
    {
        if (held_.fn == nullptr) return;
        (void)hipStreamSynchronize(stream_.get());
        Release r = held_;
        held_ = {nullptr, nullptr};
        r.fn(r.ctx);
    }
    struct Release {
        void (*fn)(void*);
        void* ctx;
    };

    std::vector<bool> key_only_;
    int32_t n_ = 0;
    DevPage in_;
    DevBuf mark_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> storage_;
    std::deque<std::vector<pa_column>> dict_copies_;
    Release held_{nullptr, nullptr};
    bool zero_copy_ = false, pending_ = false, finishing_ = false;
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
