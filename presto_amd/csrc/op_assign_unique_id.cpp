// op_assign_unique_id.cpp -- AssignUniqueIdOperator on device, and the pool of row ids its factory owns.
//
// Reference path replaced:
//   LocalExecutionPlanner.visitAssignUniqueId (…/sql/planner/LocalExecutionPlanner.java)
//   AssignUniqueIdOperator (…/operator/AssignUniqueIdOperator.java:115-162): the Factory's AtomicLong valuePool, requestValues,
//   generateIdColumn
//
// Contract (include/presto_amd.h).  Output page = input page + one BIGINT column without nulls (Page.appendColumn):
//   id = (stage_id << 54) | (task_id << 40) | row_id
// Row ids come in blocks of 2^20 out of the pool (getAndAdd), each block capped at 2^40; the first block is taken at creation, the
// next when a row finds the current one used up -- in the middle of a page where that is where it ends.  A block that would start at
// or beyond 2^40 fails the call with PA_ERR_ILLEGAL_STATE; the pool has moved on by then, as the reference's has.
//
// Where the blocks end is known on the host, so the ids of a page are a few (first row, rows, first id) segments and one small kernel
// writes them (unique_id_kernels.hpp).  The output page with the retained input page behind it is PassThroughOutput's
// (keyed_operator.hpp): a device page into a device-output operator goes out as the caller's own blocks.
#include <atomic>

#include "keyed_operator.hpp"
#include "unique_id_kernels.hpp"

// AssignUniqueIdOperator.Factory.valuePool.  Operators share the counter, not the handle: either may go first.
struct pa_unique_id_pool {
    std::shared_ptr<std::atomic<int64_t>> next;
};

namespace pa {
namespace {

constexpr int64_t kRowIdsPerRequest = (int64_t)1 << 20;   // ROW_IDS_PER_REQUEST
constexpr int64_t kMaxRowId = (int64_t)1 << 40;           // MAX_ROW_ID

// the invalid arguments of the whole descriptor first, then what the device path refuses; both before the device is asked for
void* checked_stream(const pa_assign_unique_id_desc* d, const pa_unique_id_pool* pool)
{
    PA_REQUIRE(d != nullptr && pool != nullptr, PA_ERR_INVALID_ARGUMENT, "null argument");
    PA_REQUIRE(d->input_channel_count > 0 && d->input_types != nullptr, PA_ERR_INVALID_ARGUMENT, "no input channels");
    for (int32_t c = 0; c < d->input_channel_count; c++) {
        const int32_t t = d->input_types[c];
        if (t != PA_ROW) check_carried_type(t, "pass-through");   // (an unknown type: invalid)
    }
    check_output_mem(d->output_mem);
    // (stage_id << 54) stays inside int64 below 2^9, (task_id << 40) below 2^23; a negative id would spill into the row id's 40 bits
    PA_REQUIRE(d->stage_id >= 0 && d->stage_id < (1 << 9), PA_ERR_INVALID_ARGUMENT, "stage_id does not fit (stage_id << 54)");
    PA_REQUIRE(d->task_id >= 0 && d->task_id < (1 << 23), PA_ERR_INVALID_ARGUMENT, "task_id does not fit (task_id << 40)");
    for (int32_t c = 0; c < d->input_channel_count; c++) check_carried_type(d->input_types[c], "pass-through");
    PA_REQUIRE(d->input_channel_count <= 64, PA_ERR_NOT_SUPPORTED, "1..64 input channels");
    return d->stream;
}

class AssignUniqueIdOperator : public pa_operator {
public:
    AssignUniqueIdOperator(const pa_assign_unique_id_desc* d, const pa_unique_id_pool* pool)
        : stream_(checked_stream(d, pool)), pool_(pool->next), mask_(((int64_t)d->stage_id << 54) | ((int64_t)d->task_id << 40))
    {
        channels_ = (size_t)d->input_channel_count;
        pass_.init(channels_, all_channels(channels_), {}, d->output_mem);
        request_values();
    }
    ~AssignUniqueIdOperator() override
    {
        (void)hipStreamSynchronize(stream_.get());
        pass_.release(stream_.get());
    }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }
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
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)channels_, PA_ERR_INVALID_ARGUMENT, "page does not match the input types");
        const int32_t n = page->position_count;
        if (n <= 0) return;
        hipStream_t s = stream_.get();
        // generateIdColumn, by block instead of by row: the rows the current block still covers, then the next block
        segments_.clear();
        for (int32_t row = 0; row < n;) {
            if (counter_ >= max_) request_values();
            const int32_t take = (int32_t)std::min<int64_t>(n - row, max_ - counter_);
            segments_.push_back({row, take, mask_ | counter_});
            counter_ += take;
            row += take;
        }
        pass_.stage(stager_, page, true, s);
        int64_t* ids = static_cast<int64_t*>(ids_.ensure((size_t)n * 8));
        timer.set_name("k_unique_ids");
        timer.begin(s);
        for (size_t at = 0; at < segments_.size(); at += kUniqueIdSegments) {
            UniqueIdArgs a{};
            a.ids = ids;
            a.segments = (int32_t)std::min<size_t>(kUniqueIdSegments, segments_.size() - at);
            for (int32_t k = 0; k < a.segments; k++) {
                a.first_row[k] = segments_[at + k].first_row;
                a.rows[k] = segments_[at + k].rows;
                a.first_id[k] = segments_[at + k].first_id;
            }
            launch_unique_ids(a, s);
        }
        timer.end(s);
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
        pass_.publish(n_, PA_BIGINT, ids_.ptr(), nullptr, stream_.get(), out);
        return true;
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finishing_ && !pending_; }
    void close() override
    {
        (void)hipStreamSynchronize(stream_.get());
        pass_.release(stream_.get());
    }
    int64_t memory_bytes() override { return (int64_t)(stager_.bytes() + ids_.capacity()); }

private:
    // requestValues (AssignUniqueIdOperator.java:156-161)
    void request_values()
    {
        counter_ = pool_->fetch_add(kRowIdsPerRequest);
        max_ = std::min(counter_ + kRowIdsPerRequest, kMaxRowId);
        PA_REQUIRE(counter_ < kMaxRowId, PA_ERR_ILLEGAL_STATE, "Unique row id exceeds a limit: " + std::to_string(kMaxRowId));
    }

    struct Segment {
        int32_t first_row, rows;
        int64_t first_id;
    };
    Stream stream_;
    std::shared_ptr<std::atomic<int64_t>> pool_;
    const int64_t mask_;
    int64_t counter_ = 0, max_ = 0;
    size_t channels_ = 0;
    PageStager stager_;
    PassThroughOutput pass_;
    std::vector<Segment> segments_;
    DevBuf ids_;
    int32_t n_ = 0;
    bool pending_ = false, finishing_ = false;
};

}  // namespace

pa_unique_id_pool* unique_id_pool_new(int64_t first_value)
{
    // a start other than 0 lets a caller reach the ends of blocks and the limit without 2^40 rows; beyond the limit there is nothing to start at
    PA_REQUIRE(first_value >= 0 && first_value <= kMaxRowId, PA_ERR_INVALID_ARGUMENT, "first_value outside 0 .. 2^40");
    return new pa_unique_id_pool{std::make_shared<std::atomic<int64_t>>(first_value)};
}
void unique_id_pool_delete(pa_unique_id_pool* pool) { delete pool; }
pa_operator* make_assign_unique_id(const pa_assign_unique_id_desc* desc, pa_unique_id_pool* pool) { return new AssignUniqueIdOperator(desc, pool); }

}  // namespace pa
