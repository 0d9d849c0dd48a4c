// op_topn_ranking.cpp -- TopNRankingOperator on device: row_number() / rank() OVER (PARTITION BY k ORDER BY x) <= n.
//
// Reference path replaced:
//   LocalExecutionPlanner.visitTopNRanking
//   TopNRankingOperator (…/operator/TopNRankingOperator.java) over GroupedTopNRowNumberBuilder / GroupedTopNRankBuilder, ordered by
//   SimplePageWithPositionComparator, partitions from GroupByHash.getGroupIds as RowNumberOperator (op_row_number.cpp).
//
// Contract (include/presto_amd.h).  Output only after finish: partitions in first-seen order, inside a partition in comparator order,
// rows that compare equal in arrival order; ROW_NUMBER keeps the rows numbered <= n, RANK the rows with at most n - 1 strictly smaller
// rows in their partition.  RANK peers are the rows the comparator calls equal: -0.0 and +0.0 in a sort channel are NOT peers (the
// reference finds peers with IS NOT DISTINCT FROM but orders with Double.compare, so its own result for such a partition depends on
// arrival order).
//
// State is bounded by what can still matter.  The operator holds rows in a HeldRows (held_rows.hpp) as [rows retained by the last
// prune | rows appended since]:
//   per page   group ids (DistinctHash::add_page), the image of the first sort channel (launch_topn_keys), the arrival filter
//              keep = image <= bound[gid] (topn_ranking_kernels.hpp), keep counts -> scan -> positions (KeepCompactor,
//              keyed_operator.hpp), Block.copyPositions of the survivors behind the held rows;
//   prune      when the rows appended since the last prune reach max(threshold, rows retained by it), and at finish: the held rows
//              sorted by (gid, sort channels) (row_sort.hpp), numbered / ranked, the rows kept gathered into fresh columns, bound[gid]
//              rewritten for every partition that holds n rows.
// Why the time of a prune cannot show in the result: bound[gid] is the image of a row that stands at place n of its partition, so a row
// with a greater image has n rows in front of it for good; bounds only ever tighten, and a row dropped under a looser bound would be
// dropped under a tighter one.  A prune itself drops only rows that n others strictly precede (ROW_NUMBER: in (order, arrival)).
#include <cstdlib>

#include "held_rows.hpp"
#include "keyed_operator.hpp"
#include "row_sort.hpp"
#include "topn_ranking_kernels.hpp"

namespace pa {
namespace {

constexpr int64_t kDefaultPruneRows = (int64_t)1 << 22;

// checked before the device is asked for: a shape the device path does not take is reported as such with or without a GPU
void* checked_stream(const pa_topn_ranking_desc* d)
{
    PA_REQUIRE(d != nullptr && d->input_types != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    const int32_t channels = d->input_channel_count;
    const int32_t* types = d->input_types;
    check_input_channels(channels);
    PA_REQUIRE(d->ranking_type == PA_RANKING_ROW_NUMBER || d->ranking_type == PA_RANKING_RANK || d->ranking_type == PA_RANKING_DENSE_RANK,
               PA_ERR_INVALID_ARGUMENT, "unknown ranking_type");
    PA_REQUIRE(d->max_row_count_per_partition > 0, PA_ERR_INVALID_ARGUMENT, "max_row_count_per_partition must be positive");
    PA_REQUIRE(d->partial == 0 || d->partial == 1, PA_ERR_INVALID_ARGUMENT, "partial is 0 or 1");
    PA_REQUIRE(d->output_channel_count >= 0 && (d->output_channel_count == 0 || d->output_channels != nullptr), PA_ERR_INVALID_ARGUMENT, "no output channels");
    PA_REQUIRE(d->partition_channel_count >= 0 && (d->partition_channel_count == 0 || d->partition_channels != nullptr), PA_ERR_INVALID_ARGUMENT,
               "partition channels are null");
    PA_REQUIRE(d->sort_channel_count > 0 && d->sort_channels != nullptr && d->sort_orders != nullptr, PA_ERR_INVALID_ARGUMENT, "no sort channels");
    check_channels(d->output_channels, d->output_channel_count, channels, "output");
    // (a channel out of range is reported before a count the device path does not take: of a longer list, the first channels only)
    check_channels(d->partition_channels, std::min(d->partition_channel_count, kMaxJoinChannels + 1), channels, "partition");
    for (int32_t i = 0; i < d->sort_channel_count; i++) {
        check_channels(d->sort_channels + i, 1, channels, "sort");
        PA_REQUIRE(d->sort_orders[i] >= 0 && d->sort_orders[i] <= 3, PA_ERR_INVALID_ARGUMENT, "unknown sort order");
    }
    check_hash_channel(d->hash_channel, channels, types);
    PA_REQUIRE(d->expected_positions >= 0, PA_ERR_INVALID_ARGUMENT, "expected_positions is negative");
    check_output_mem(d->output_mem);
    // what the device path does not take
    PA_REQUIRE(d->ranking_type != PA_RANKING_DENSE_RANK, PA_ERR_NOT_SUPPORTED, "dense_rank (the reference does not take it either)");
    PA_REQUIRE(d->output_channel_count <= 64, PA_ERR_NOT_SUPPORTED, "more output channels than the device path takes");
    PA_REQUIRE(d->sort_channel_count <= 64, PA_ERR_NOT_SUPPORTED, "more sort channels than the device path takes");
    PA_REQUIRE(d->partition_channel_count <= kMaxJoinChannels, PA_ERR_NOT_SUPPORTED, "more partition channels than the device path takes");
    for (int32_t i = 0; i < d->output_channel_count; i++) {
        const int32_t t = types[d->output_channels[i]];
        // the rows kept are copied position by position: no such copy for 16-byte values and rows
        PA_REQUIRE(t != PA_LONG_DECIMAL && t != PA_ROW, PA_ERR_NOT_SUPPORTED, "long decimal / row output channels");
    }
    for (int32_t i = 0; i < d->partition_channel_count; i++) check_key_type(types[d->partition_channels[i]], "partition");
    for (int32_t i = 0; i < d->sort_channel_count; i++) {
        switch (types[d->sort_channels[i]]) {
            case PA_BIGINT:
            case PA_INTEGER:
            case PA_DATE:
            case PA_DOUBLE:
            case PA_REAL:
            case PA_BOOLEAN:
            case PA_VARCHAR: break;
            case PA_DECIMAL:   // (a short decimal is declared BIGINT for sorts, as for TopN / OrderBy)
            case PA_LONG_DECIMAL:
            case PA_ROW: throw Error(PA_ERR_NOT_SUPPORTED, "sort channel type not supported on the device");
            default: throw Error(PA_ERR_INVALID_ARGUMENT, "unknown sort channel type");
        }
    }
    return d->stream;
}

class TopNRankingOperator : public pa_operator {
public:
    explicit TopNRankingOperator(const pa_topn_ranking_desc* d)
        : stream_(checked_stream(d)), limit_(d->max_row_count_per_partition), rank_(d->ranking_type == PA_RANKING_RANK), partial_(d->partial != 0)
    {
        types_.assign(d->input_types, d->input_types + d->input_channel_count);
        output_channels_.assign(d->output_channels, d->output_channels + d->output_channel_count);
        partition_channels_.assign(d->partition_channels, d->partition_channels + d->partition_channel_count);
        sort_channels_.assign(d->sort_channels, d->sort_channels + d->sort_channel_count);
        sort_orders_.assign(d->sort_orders, d->sort_orders + d->sort_channel_count);
        output_mem_ = d->output_mem;
        needed_.assign(types_.size(), false);
        kept_channel_.assign(types_.size(), false);
        for (int32_t c : partition_channels_) needed_[c] = true;
        for (int32_t c : sort_channels_) needed_[c] = kept_channel_[c] = true;
        for (int32_t c : output_channels_) needed_[c] = kept_channel_[c] = true;
        held_.init(types_, kept_channel_);
        // (read per operator, so that a test can change it between operators of one process)
        if (const char* e = getenv("PRESTO_AMD_TOPN_RANKING_PRUNE_ROWS")) {
            const long long v = atoll(e);
            if (v > 0) threshold_ = v;
        }
        hipStream_t s = stream_.get();
        hash_ = make_distinct_hash(types_, partition_channels_, d->expected_positions, s);
        grow_bounds(1, s);
        timer.set_name("k_topn_ranking_filter");
    }
    ~TopNRankingOperator() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }

    void stats(int64_t* partitions, int64_t* capacity, int64_t* rows_held)
    {
        if (partitions) *partitions = hash_ ? hash_->settle(stream_.get()) : 1;
        if (capacity) *capacity = hash_ ? hash_->capacity() : 0;
        if (rows_held) *rows_held = held_.rows;
    }

    bool needs_input() override { return !finishing_; }
    bool is_finished() override { return finishing_ && (done_ || held_.rows == 0); }
    void finish() override { finishing_ = true; }

    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(!finishing_, PA_ERR_ILLEGAL_STATE, "Operator is already finishing");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int32_t n = page->position_count;
        if (n <= 0) return;
        hipStream_t s = stream_.get();
        const DevPage in = stager_.stage(page, &needed_, s);
        for (size_t c = 0; c < types_.size(); c++)
            if (needed_[c]) PA_REQUIRE(in.cols[c].type == types_[c], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared input type");
        // group ids in first-seen order; one partition: id 0
        uint64_t* gids = static_cast<uint64_t*>(gids_.ensure((size_t)n * 8));
        if (hash_) {
            uint8_t* mark = static_cast<uint8_t*>(mark_.ensure(((size_t)n + 3) & ~(size_t)3));
            hash_->add_page(KeyColumns(in, partition_channels_).cols, n, mark, nullptr, 0, table_timer_, s, gids);
        }
        else PA_HIP(hipMemsetAsync(gids, 0, (size_t)n * 8, s));
        // the first sort channel's image with its NULL placement folded in: image order never contradicts comparator order
        const DevColumn& first = in.cols[sort_channels_[0]];
        uint64_t* images = static_cast<uint64_t*>(images_.ensure((size_t)n * 8));
        launch_topn_keys(first.type, first.values, first.offsets, first.nulls, n, sort_orders_[0], images, s);
        // The page goes through the filter in slices of about the prune threshold: while a partition's bound is still open every row of
        // it survives, so a page far larger than the threshold would be appended -- and sorted -- whole; after the first slice's prune
        // the bounds stand and the rest of the page loses at the filter.  (Slices start at multiples of 1024 rows: 16-byte loads.)
        const int64_t step = (std::max<int64_t>(threshold_, 1024) + 1023) / 1024 * 1024;
        uint8_t* keep = static_cast<uint8_t*>(keep_.ensure(((size_t)std::min<int64_t>(n, step) + 3) & ~(size_t)3));
        for (int64_t at = 0; at < n; at += step) {
            const int32_t m = (int32_t)std::min<int64_t>(step, n - at);
            timer.begin(s);
            launch_topn_ranking_filter(gids + at, images + at, bound_.as<uint64_t>(), bound_n_, m, keep, s);
            timer.end(s);
            int32_t kept = 0;
            const int32_t* positions = kept_rows_.positions_of(keep, m, &kept, "topn ranking", s);
            if (kept > 0) {
                if (held_.rows + kept > INT32_MAX) prune(s);
                PA_REQUIRE(held_.rows + kept <= INT32_MAX, PA_ERR_INSUFFICIENT_RESOURCES, "more rows held than one sort takes");
                append(slice_of(in, at), gids + at, positions, kept, s);
            }
            if (appended_ >= std::max(threshold_, retained_)) prune(s);
        }
        // the page's buffers are the caller's again, and the stager's are reused by the next page
        PA_HIP(hipStreamSynchronize(s));
    }

    bool get_output(pa_page* out) override
    {
        if (!finishing_ || done_) return false;
        done_ = true;
        if (held_.rows == 0) return false;
        hipStream_t s = stream_.get();
        // a prune leaves the held rows in output order and their ranking in ranking_kept_: nothing to do when none arrived since the last
        if (appended_ > 0) prune(s);
        const size_t nc = output_channels_.size();
        out_cols_.clear();
        out_cols_.resize(nc + (partial_ ? 0 : 1));
        for (size_t c = 0; c < nc; c++) view_column(out_cols_[c], held_.view(output_channels_[c]));
        if (!partial_) {
            DevColumn ranking;   // BIGINT, flat, no nulls
            ranking.values = ranking_kept_.ptr();
            view_column(out_cols_[nc], ranking);
        }
        publish_output(out_cols_, (int32_t)held_.rows, output_mem_, s, out, storage_);
        return true;
    }

    void close() override { (void)hipStreamSynchronize(stream_.get()); }

    // table + key store + held rows, and the scratch of a page / a prune while it is allocated
    int64_t memory_bytes() override
    {
        size_t b = stager_.bytes() + gids_.capacity() + images_.capacity() + mark_.capacity() + keep_.capacity() + kept_rows_.bytes() + gather_.bytes() + held_gids_.capacity() + bound_.capacity() + run_start_.capacity() +
                   ranking_kept_.capacity() + sorter_.bytes() + varchar_tmp_.values.capacity() + varchar_tmp_.offsets.capacity() + varchar_tmp_.nulls.capacity();
        return (hash_ ? hash_->memory_bytes() : 0) + (int64_t)(b + held_.bytes());
    }

private:
    // the rows of a staged page from row `at` on (VARCHAR offsets index the page's bytes: the values stay where they are)
    static DevPage slice_of(const DevPage& in, int64_t at)
    {
        if (at == 0) return in;
        DevPage out = in;
        out.n = in.n - (int32_t)at;
        for (DevColumn& c : out.cols) {
            if (c.values == nullptr) continue;
            if (c.varwidth) c.offsets += at;
            else c.values = static_cast<const char*>(c.values) + (size_t)at * (size_t)type_width(c.type);
            if (c.nulls) c.nulls += at;
        }
        return out;
    }

    // bound[] by group id, ~0 for partitions that do not hold n rows yet
    void grow_bounds(int64_t partitions, hipStream_t s) { grow_by_group_id(bound_, &bound_n_, partitions, 0xff, s); }

    // Block.copyPositions of the page's survivors behind the held rows, with their group ids
    void append(const DevPage& in, const uint64_t* gids, const int32_t* positions, int32_t k, hipStream_t s)
    {
        const int64_t rows = held_.rows;
        held_.append_positions(in, positions, k, gather_, varchar_tmp_, s);
        uint64_t* hg = static_cast<uint64_t*>(held_gids_.reserve_keep((size_t)(rows + k) * 8, (size_t)rows * 8, s));
        launch_gather_flat(gids, 8, positions, k, hg + rows, s);
        appended_ += k;
    }

    // sort the held rows by (gid, sort channels), number / rank them, keep what can still matter, rewrite the bounds
    void prune(hipStream_t s)
    {
        const int64_t n = held_.rows;
        if (n == 0) return;
        const int64_t partitions = hash_ ? hash_->settle(s) : 1;
        grow_bounds(partitions, s);
        std::vector<DevColumn> cols;
        for (int32_t c : sort_channels_) cols.push_back(held_.view(c));
        // The held array is [retained | appended]: the retained rows are in (gid, order, arrival) order and arrived before every
        // appended row, and appended rows stand in arrival order.  So array order is arrival order inside every class of rows that
        // compare equal, and the stable sort keeps it there: no sequence column is needed.
        const int32_t* perm = sorter_.sort(cols, sort_orders_, hash_ ? held_gids_.as<uint64_t>() : nullptr, bits_for(partitions), n, s);
        DevBuf sorted_gids_buf, images_buf, ranking_buf, keep_buf, differs_buf, peer_flag_buf, peer_index_buf, peer_start_buf, rowids_buf;
        const uint64_t* sorted_gids = held_gids_.as<uint64_t>();   // one partition: all 0 in any order
        if (hash_) {
            uint64_t* sg = static_cast<uint64_t*>(sorted_gids_buf.ensure((size_t)n * 8));
            launch_gather_flat(held_gids_.ptr(), 8, perm, n, sg, s);
            sorted_gids = sg;
        }
        int32_t* run_start = static_cast<int32_t*>(run_start_.ensure((size_t)bound_n_ * 4));
        TopNRankingRankArgs a;
        memset(&a, 0, sizeof a);
        if (rank_) {
            // peer runs: a row opens one when it differs from the sorted row before it on any sort channel
            uint8_t* differs = static_cast<uint8_t*>(differs_buf.ensure((size_t)n));
            PA_HIP(hipMemsetAsync(differs, 0, (size_t)n, s));
            for (const DevColumn& c : cols) launch_topn_ranking_differs(c.type, c.values, c.offsets, c.nulls, perm, (int32_t)n, differs, s);
            int32_t* peer_flag = static_cast<int32_t*>(peer_flag_buf.ensure((size_t)n * 4));
            int32_t* peer_index = static_cast<int32_t*>(peer_index_buf.ensure((size_t)n * 4));
            int32_t* peer_start = static_cast<int32_t*>(peer_start_buf.ensure((size_t)n * 4));
            launch_topn_ranking_heads(sorted_gids, differs, (int32_t)n, run_start, bound_n_, peer_flag, s);
            launch_exclusive_scan_i32(peer_flag, peer_index, n, static_cast<int32_t*>(kept_rows_.total.ensure(64)), kept_rows_.scan_temp.ensure(scan_temp_bytes(n)), s);
            launch_topn_ranking_peer_starts(peer_flag, peer_index, (int32_t)n, peer_start, s);
            a.peer_flag = peer_flag;
            a.peer_index = peer_index;
            a.peer_start = peer_start;
        }
        else launch_topn_ranking_heads(sorted_gids, nullptr, (int32_t)n, run_start, bound_n_, nullptr, s);
        uint64_t* images = static_cast<uint64_t*>(images_buf.ensure((size_t)n * 8));
        launch_topn_keys(cols[0].type, cols[0].values, cols[0].offsets, cols[0].nulls, n, sort_orders_[0], images, s);
        a.sorted_gids = sorted_gids;
        a.perm = perm;
        a.images = images;
        a.run_start = run_start;
        a.run_start_n = bound_n_;
        a.limit = limit_;
        a.bound = bound_.as<uint64_t>();
        a.bound_n = bound_n_;
        a.ranking = static_cast<int64_t*>(ranking_buf.ensure((size_t)n * 8));
        a.keep = static_cast<uint8_t*>(keep_buf.ensure(((size_t)n + 3) & ~(size_t)3));
        a.n = (int32_t)n;
        launch_topn_ranking_rank(a, s);
        int32_t kept = 0;
        const int32_t* sorted_positions = kept_rows_.positions_of(a.keep, (int32_t)n, &kept, "topn ranking", s);
        PA_REQUIRE(kept > 0, PA_ERR_DEVICE, "topn ranking: a prune kept nothing");
        int32_t* rowids = static_cast<int32_t*>(rowids_buf.ensure((size_t)kept * 4));
        launch_gather_flat(perm, 4, sorted_positions, kept, rowids, s);
        // the rows kept into fresh columns, in output order
        held_.keep_positions(rowids, kept, gather_, s);
        DevBuf fresh_gids;
        launch_gather_flat(sorted_gids, 8, sorted_positions, kept, fresh_gids.ensure((size_t)kept * 8), s);
        launch_gather_flat(a.ranking, 8, sorted_positions, kept, ranking_kept_.ensure((size_t)kept * 8), s);
        PA_HIP(hipStreamSynchronize(s));
        held_gids_ = std::move(fresh_gids);
        sorter_.release();
        retained_ = kept;
        appended_ = 0;
    }

    Stream stream_;
    PageStager stager_;
    std::unique_ptr<DistinctHash> hash_;   // null: no partition channels
    KernelTimer table_timer_;              // (the table's passes are timed apart: pa_op_kernel_time reports the arrival filter)
    std::vector<int32_t> types_, output_channels_, partition_channels_, sort_channels_, sort_orders_;
    std::vector<bool> needed_, kept_channel_;   // staged per page; held (sort and output channels)
    const int64_t limit_;
    const bool rank_, partial_;
    int64_t threshold_ = kDefaultPruneRows;
    int32_t output_mem_ = PA_MEM_HOST;
    // the rows held: [retained | appended], by input channel, with their group ids
    HeldRows held_;
    DevBuf held_gids_;
    int64_t retained_ = 0, appended_ = 0;
    DevBuf bound_, run_start_;
    int64_t bound_n_ = 0;
    DevBuf gids_, images_, mark_, keep_, ranking_kept_;
    KeepCompactor kept_rows_;   // (its scan scratch also serves the scan of the peer flags in a prune)
    PositionGather gather_;
    OutColumn varchar_tmp_;
    RowSorter sorter_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> storage_;
    bool finishing_ = false, done_ = false;
};

}  // namespace

pa_operator* make_topn_ranking(const pa_topn_ranking_desc* desc) { return new TopNRankingOperator(desc); }
void topn_ranking_stats(pa_operator* op, int64_t* partitions, int64_t* capacity, int64_t* rows_held)
{
    TopNRankingOperator* r = dynamic_cast<TopNRankingOperator*>(op);
    PA_REQUIRE(r != nullptr, PA_ERR_INVALID_ARGUMENT, "not a TopNRanking operator");
    r->stats(partitions, capacity, rows_held);
}

}  // namespace pa
