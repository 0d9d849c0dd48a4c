// op_row_number.cpp -- RowNumberOperator on device: row_number() OVER (PARTITION BY k), with an optional cap of rows per partition.
//
// Reference path replaced:
//   LocalExecutionPlanner.visitRowNumber (…/sql/planner/LocalExecutionPlanner.java:900-938)
//   RowNumberOperator (…/operator/RowNumberOperator.java: state machine :183-209, getRowsWithRowNumber :289-299, getSelectedRows :313-342)
// over GroupByHash.getGroupIds, as MarkDistinctOperator and DistinctLimitOperator (op_distinct.cpp).
//
// Contract (include/presto_amd.h).  The partition of a row is its group under IS NOT DISTINCT FROM over the partition channels.  Rows are
// taken in page order: a row gets count[partition] + 1 and the count goes up by one, counts carried for the operator's life.  Without a
// cap the output page is the input's output channels with that BIGINT column behind them.  With a cap m a row whose partition already
// stands at m is dropped and does not count; the rows kept come out compacted, in input order.  No partition channels: one partition,
// no table.
//
// Per page with partition channels: DistinctHash::add_page with group ids (canon -> insert -> mark -> scan -> publish -> ids), a stable
// sort of (id, position) over the bits the distinct count needs, the rank and update passes of row_number_kernels.hpp; with a cap the
// keep marks -> counts -> scan -> positions (KeepCompactor) -> Block.copyPositions of every output channel and of the row numbers.
// Without a cap the output page, with the retained input page behind it, is PassThroughOutput's (both in keyed_operator.hpp).
#include "keyed_operator.hpp"
#include "sort_kernels.hpp"

namespace pa {
namespace {

// checked before the device is asked for: a shape the device path does not take is reported as such with or without a GPU
void* checked_stream(const pa_row_number_desc* d)
{
    PA_REQUIRE(d != nullptr && d->input_types != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    const int32_t channels = d->input_channel_count;
    const int32_t* types = d->input_types;
    check_input_channels(channels);
    PA_REQUIRE(d->max_rows_per_partition >= -1, PA_ERR_INVALID_ARGUMENT, "max_rows_per_partition is negative (-1 = absent)");
    PA_REQUIRE(d->output_channel_count >= 0 && (d->output_channel_count == 0 || d->output_channels != nullptr), PA_ERR_INVALID_ARGUMENT, "no output channels");
    PA_REQUIRE(d->output_channel_count <= 64, PA_ERR_NOT_SUPPORTED, "more output channels than the device path takes");
    for (int32_t i = 0; i < d->output_channel_count; i++) {
        const int32_t c = d->output_channels[i];
        check_channels(&c, 1, channels, "output");
        // under a cap the rows kept are copied out position by position: no such copy for 16-byte values and rows
        PA_REQUIRE(d->max_rows_per_partition < 0 || (types[c] != PA_LONG_DECIMAL && types[c] != PA_ROW), PA_ERR_NOT_SUPPORTED,
                   "long decimal / row output channels under max_rows_per_partition");
    }
    PA_REQUIRE(d->partition_channel_count >= 0 && (d->partition_channel_count == 0 || d->partition_channels != nullptr), PA_ERR_INVALID_ARGUMENT,
               "partition channels are null");
    PA_REQUIRE(d->partition_channel_count <= kMaxJoinChannels, PA_ERR_NOT_SUPPORTED, "more partition channels than the device path takes");
    check_key_channels(d->partition_channels, d->partition_channel_count, channels, types, "partition");
    check_hash_channel(d->hash_channel, channels, types);
    PA_REQUIRE(d->expected_positions >= 0, PA_ERR_INVALID_ARGUMENT, "expected_positions is negative");
    check_output_mem(d->output_mem);
    return d->stream;
}

class RowNumberOperator : public pa_operator {
public:
    explicit RowNumberOperator(const pa_row_number_desc* d) : stream_(checked_stream(d)), cap_(d->max_rows_per_partition)
    {
        types_.assign(d->input_types, d->input_types + d->input_channel_count);
        output_channels_.assign(d->output_channels, d->output_channels + d->output_channel_count);
        partition_channels_.assign(d->partition_channels, d->partition_channels + d->partition_channel_count);
        output_mem_ = d->output_mem;
        pass_.init(types_.size(), output_channels_, partition_channels_, output_mem_);
        hash_ = make_distinct_hash(types_, partition_channels_, d->expected_positions, stream_.get());
    }
    ~RowNumberOperator() override
    {
        (void)hipStreamSynchronize(stream_.get());
        pass_.release(stream_.get());
    }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }
    // without a cap the output page may be the input page's own blocks: a retained input page is let go once its output page is
    bool takes_retained() override { return true; }

    void stats(int64_t* partition_count, int64_t* table_capacity)
    {
        if (partition_count) *partition_count = hash_ ? hash_->settle(stream_.get()) : 1;
        if (table_capacity) *table_capacity = hash_ ? hash_->capacity() : 0;
    }

    // RowNumberOperator.java:183-209; the single partition under a cap is done once the cap is reached
    bool needs_input() override
    {
        if (!pending_) pass_.release(stream_.get());
        return !finishing_ && !pending_ && !single_full();
    }
    bool is_finished() override { return !pending_ && (finishing_ || single_full()); }
    void finish() override { finishing_ = true; }

    void add_input(const pa_page* page) override
    {
        pass_.release(stream_.get());
        pass_.hold(page);
        PA_REQUIRE(!finishing_ && !pending_ && !single_full(), PA_ERR_ILLEGAL_STATE, "Operator does not need input");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int32_t n = page->position_count;
        if (n <= 0) return;
        hipStream_t s = stream_.get();
        // getRowsWithRowNumber: the input blocks as they are where they can stay (their encodings included), the row numbers behind them;
        // under a cap the rows kept are copied out
        const DevPage& in = pass_.stage(stager_, page, cap_ < 0, s);
        int64_t* rn = static_cast<int64_t*>(rn_.ensure((size_t)n * 8));
        int32_t kept = n;
        const int32_t* positions = nullptr;
        if (!hash_) {
            launch_row_number_iota(single_count_, n, rn, s);
            if (cap_ >= 0) {
                kept = (int32_t)std::min<int64_t>(n, cap_ - single_count_);
                if (kept < n) {   // a prefix of the page (kept > 0: the operator needed input)
                    int32_t* p = static_cast<int32_t*>(kept_rows_.positions.ensure((size_t)kept * 4));
                    launch_row_number_positions_iota(kept, p, s);
                    positions = p;
                }
            }
            single_count_ += kept;
        }
        else {
            number_partitioned(in, n, rn, s);
            if (cap_ >= 0) positions = kept_rows_.positions_of(keep_.as<uint8_t>(), n, &kept, "row number", s);
        }
        if (kept == 0) return;   // a page that keeps no row produces no page
        if (cap_ >= 0) {
            // getSelectedRows: Block.copyPositions of every output channel (a page kept whole is copied too: the blocks are the
            // operator's own either way), then the row numbers
            if (positions == nullptr) {
                int32_t* p = static_cast<int32_t*>(kept_rows_.positions.ensure((size_t)kept * 4));
                launch_row_number_positions_iota(kept, p, s);
                positions = p;
            }
            out_cols_.resize(output_channels_.size() + 1);
            // (no 2 GiB message: the rows kept, each once, of ONE staged block -- under 2 GiB, PageStager::stage)
            for (size_t c = 0; c < output_channels_.size(); c++) gather_.copy_positions(in.cols[output_channels_[c]], positions, kept, out_cols_[c], s);
            OutColumn& o = out_cols_.back();
            o.type = PA_BIGINT;
            o.varwidth = o.has_nulls = o.is_view = o.host_ready = false;
            launch_gather_flat(rn, 8, positions, kept, o.values.ensure((size_t)kept * 8), s);
            // (the copies read the caller's page: as in DistinctLimitOperator they are done when the call returns unless the page
            // lives in HBM and stays there)
            if (page->mem != PA_MEM_DEVICE || output_mem_ != PA_MEM_DEVICE) PA_HIP(hipStreamSynchronize(s));
        }
        n_ = kept;
        pending_ = true;
    }

    bool get_output(pa_page* out) override
    {
        if (!pending_) {
            pass_.release(stream_.get());
            return false;
        }
        pending_ = false;
        if (cap_ < 0) pass_.publish(n_, PA_BIGINT, rn_.ptr(), nullptr, stream_.get(), out);
        else publish_output(out_cols_, n_, output_mem_, stream_.get(), out, storage_);
        return true;
    }

    void close() override
    {
        (void)hipStreamSynchronize(stream_.get());
        pass_.release(stream_.get());
    }
    int64_t memory_bytes() override
    {
        size_t b = stager_.bytes() + rn_.capacity() + counts_.capacity() + gids_.capacity() + sorted_gids_.capacity() + sorted_rows_.capacity() +
                   rows_scratch_.capacity() + sort_temp_.capacity() + mark_.capacity() + keep_.capacity() + kept_rows_.bytes() + gather_.bytes();
        if (cap_ >= 0)
            for (const OutColumn& o : out_cols_) b += o.values.capacity() + o.offsets.capacity() + o.nulls.capacity();
        return (hash_ ? hash_->memory_bytes() : 0) + (int64_t)b;
    }

private:
    bool single_full() const { return !hash_ && cap_ >= 0 && single_count_ >= cap_; }

    // group ids -> stable sort of (id, position) -> rank -> update
    void number_partitioned(const DevPage& in, int32_t n, int64_t* rn, hipStream_t s)
    {
        uint8_t* mark = static_cast<uint8_t*>(mark_.ensure(((size_t)n + 3) & ~(size_t)3));
        uint64_t* gids = static_cast<uint64_t*>(gids_.ensure((size_t)n * 8));
        timer.set_name(hash_->add_page(KeyColumns(in, partition_channels_).cols, n, mark, nullptr, 0, timer, s, gids));
        // the partitions seen so far, exact (the wait the sort's bit range is worth: with 4 partitions it is 2 bits, not the 24 an
        // upper bound of a 2^24-row page would give); every id of the page is below it
        const int64_t partitions = hash_->settle(s);
        grow_by_group_id(counts_, &counts_n_, partitions, 0, s);   // counts by group id; new entries are zero
        uint64_t* sorted_gids = static_cast<uint64_t*>(sorted_gids_.ensure((size_t)n * 8));
        int32_t* sorted_rows = static_cast<int32_t*>(sorted_rows_.ensure((size_t)n * 4));
        int32_t* rows_scratch = static_cast<int32_t*>(rows_scratch_.ensure((size_t)n * 4));
        const size_t temp_bytes = sort_pairs_temp_bytes(n);
        void* temp = sort_temp_.ensure(temp_bytes);
        launch_sort_pairs(gids, nullptr, rows_scratch, sorted_gids, sorted_rows, n, 0, bits_for(partitions), temp, temp_bytes, s);
        RowNumberRankArgs a;
        memset(&a, 0, sizeof a);
        a.gids = sorted_gids;
        a.rows = sorted_rows;
        a.counts = counts_.as<int64_t>();
        a.counts_n = counts_n_;
        a.cap = cap_;
        a.rn = rn;
        a.keep = cap_ >= 0 ? static_cast<uint8_t*>(keep_.ensure(((size_t)n + 3) & ~(size_t)3)) : nullptr;
        a.tails = reinterpret_cast<int64_t*>(gids);   // (the unsorted ids have been read for the last time: the sort is enqueued)
        a.n = n;
        launch_row_number_rank(a, s);
        launch_row_number_update(sorted_gids, a.tails, n, cap_, counts_.as<int64_t>(), counts_n_, s);
    }

    Stream stream_;
    PageStager stager_;
    std::unique_ptr<DistinctHash> hash_;   // null: no partition channels
    std::vector<int32_t> types_, output_channels_, partition_channels_;
    int64_t cap_ = -1, single_count_ = 0, counts_n_ = 0;
    int32_t output_mem_ = PA_MEM_HOST, n_ = 0;
    PassThroughOutput pass_;   // without a cap: the output page; with one: the staged page and the retained one
    DevBuf rn_, counts_, gids_, sorted_gids_, sorted_rows_, rows_scratch_, sort_temp_, mark_, keep_;
    KeepCompactor kept_rows_;
    PositionGather gather_;
    std::vector<OutColumn> out_cols_;   // under a cap: the rows kept, copied out
    std::vector<pa_column> storage_;
    bool pending_ = false, finishing_ = false;
};

}  // namespace

pa_operator* make_row_number(const pa_row_number_desc* desc) { return new RowNumberOperator(desc); }
void row_number_stats(pa_operator* op, int64_t* partition_count, int64_t* table_capacity)
{
    RowNumberOperator* r = dynamic_cast<RowNumberOperator*>(op);
    PA_REQUIRE(r != nullptr, PA_ERR_INVALID_ARGUMENT, "not a RowNumber operator");
    r->stats(partition_count, table_capacity);
}

}  // namespace pa
