// op_order_by.cpp -- OrderByOperator (core/trino-main/src/main/java/io/trino/operator/OrderByOperator.java:45-330): collect every
// input page (PagesIndex.addPage), sort by (sortChannels, sortOrders) when the input ends (PagesIndex.sort ->
// PagesIndexOrdering with SimplePagesIndexComparator), emit the output channels in order.
//
// The reference quick-sorts row addresses with a multi-channel comparator.  Here the rows are collected in a HeldRows
// (held_rows.hpp), a RowSorter (row_sort.hpp) sorts a row permutation over its columns -- stable, so fully tied rows keep
// arrival order -- and the output channels are gathered out of the HeldRows through the permutation.  What this file adds to
// the sort: pages that stay where they are are listed instead of copied (one alone is sorted in place); flat 4- / 8-byte
// output channels without NULL rows are offered to the sorter as riding payload (SortCarry) and taken from it when they rode;
// a first sort channel of integers without NULL rows that is also an output channel is written from the sorted images.
#include <algorithm>
#include <cstring>

#include "held_rows.hpp"
#include "keyed_operator.hpp"
#include "operator.hpp"
#include "row_sort.hpp"
#include "static_kernels.hpp"

namespace pa {

namespace {

class OrderByOperator : public pa_operator {
public:
    explicit OrderByOperator(const pa_order_by_desc* d) : stream_(d->stream)
    {
        require_device();
        PA_REQUIRE(d->input_channel_count > 0 && d->input_types, PA_ERR_INVALID_ARGUMENT, "OrderBy needs input types");
        PA_REQUIRE(d->sort_channel_count > 0 && d->sort_channels && d->sort_orders, PA_ERR_INVALID_ARGUMENT, "OrderBy needs sort channels");
        types_.assign(d->input_types, d->input_types + d->input_channel_count);
        if (d->output_channels) output_channels_.assign(d->output_channels, d->output_channels + d->output_channel_count);
        sort_channels_.assign(d->sort_channels, d->sort_channels + d->sort_channel_count);
        sort_orders_.assign(d->sort_orders, d->sort_orders + d->sort_channel_count);
        for (int c : output_channels_) PA_REQUIRE(c >= 0 && c < (int)types_.size(), PA_ERR_INVALID_ARGUMENT, "output channel out of range");
        for (size_t i = 0; i < sort_channels_.size(); i++) {
            PA_REQUIRE(sort_channels_[i] >= 0 && sort_channels_[i] < (int)types_.size(), PA_ERR_INVALID_ARGUMENT, "sort channel out of range");
            PA_REQUIRE(sort_orders_[i] >= 0 && sort_orders_[i] <= 3, PA_ERR_INVALID_ARGUMENT, "unknown sort order");
        }
        // what the device path does not take, said before a row arrives: a sort channel needs an order-preserving image, an output
        // channel a copy by position (channels that are neither are never read)
        for (int c : sort_channels_) check_key_type(types_[(size_t)c], "sort");
        for (int c : output_channels_) check_carried_type(types_[(size_t)c], "output");
        output_mem_ = d->output_mem;
        needed_.assign(types_.size(), false);
        for (int c : output_channels_) needed_[(size_t)c] = true;
        for (int c : sort_channels_) needed_[(size_t)c] = true;
        store_.init(types_, needed_);
    }
    ~OrderByOperator() override
    {
        (void)hipStreamSynchronize(stream_.get());
        for (Held& h : held_) {
            if (h.release) h.release(h.release_ctx);
        }
    }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }

    bool needs_input() override { return !finishing_; }

    bool takes_retained() override { return true; }

    // PagesIndex.addPage keeps the Page; so does this for device pages that stay where they are (PA_PAGE_STABLE, PA_PAGE_RETAINED) and
    // hold only flat fixed-width blocks in the needed channels: they are listed, not copied.  One such page alone is sorted in place; several
    // are laid behind each other when the input ends (the same copies, later).  Every other page is copied when it arrives -- its
    // buffers are the caller's again when add_input returns -- after the pages listed before it.
    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(!finishing_, PA_ERR_ILLEGAL_STATE, "Operator is already finishing");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the operator's input types");
        const bool retained = (page->flags & PA_PAGE_RETAINED) != 0 && page->release != nullptr;
        if (page->position_count == 0) {
            if (retained) page->release(page->release_ctx);
            return;
        }
        const int64_t m = page->position_count;
        if (store_.rows + m > INT32_MAX) {
            if (retained) page->release(page->release_ctx);   // (nothing of it was read)
            throw Error(PA_ERR_INSUFFICIENT_RESOURCES, "too many rows for one sort");
        }
        if (page->mem == PA_MEM_DEVICE && (retained || (page->flags & PA_PAGE_STABLE) != 0) && holdable(page)) {
            Held h;
            h.rows = m;
            h.cols.assign(page->columns, page->columns + page->channel_count);
            if (retained) {
                h.release = page->release;
                h.release_ctx = page->release_ctx;
            }
            held_.push_back(std::move(h));
            store_.rows += m;
            return;
        }
        // (a retained page that is copied goes back to its owner when the copies have run -- also when a check below throws)
        struct ReleaseAtExit {
            const pa_page* p;
            bool on;
            hipStream_t s;
            ~ReleaseAtExit()
            {
                if (!on) return;
                (void)hipStreamSynchronize(s);
                p->release(p->release_ctx);
            }
        } release_at_exit{page, retained, stream_.get()};
        flush_held();
        hipStream_t s = stream_.get();
        DevPage dp = stager_.stage(page, &needed_, s);
        store_.append_page(dp, dp.n, s);
        PA_HIP(hipStreamSynchronize(s));  // the stager's buffers are reused by the next page
    }

    bool holdable(const pa_page* page) const
    {
        for (size_t c = 0; c < types_.size(); c++) {
            if (!needed_[c]) continue;
            const pa_column& in = page->columns[c];
            if (in.encoding != PA_FLAT || in.type != types_[c] || in.values == nullptr || type_width(in.type) <= 0) return false;
        }
        return true;
    }

    // the listed pages behind the rows copied so far, in arrival order; their owners get them back
    void flush_held()
    {
        if (held_.empty()) return;
        hipStream_t s = stream_.get();
        for (const Held& h : held_) store_.rows -= h.rows;   // (append_page counts them again)
        std::vector<Held> held;
        held.swap(held_);
        struct ReleaseAll {
            std::vector<Held>& held;
            hipStream_t s;
            ~ReleaseAll()
            {
                (void)hipStreamSynchronize(s);
                for (Held& h : held) {
                    if (h.release) h.release(h.release_ctx);
                }
            }
        } release_all{held, s};
        for (const Held& h : held) {
            DevPage dp;
            dp.n = (int32_t)h.rows;
            dp.cols.resize(types_.size());
            for (size_t c = 0; c < types_.size(); c++) {
                dp.cols[c].type = types_[c];
                if (!needed_[c]) continue;
                dp.cols[c].values = h.cols[c].values;
                dp.cols[c].nulls = h.cols[c].nulls;
            }
            store_.append_page(dp, dp.n, s);
        }
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finishing_ && output_done_; }

    bool get_output(pa_page* out) override
    {
        if (!finishing_ || output_done_) return false;
        output_done_ = true;
        if (store_.rows == 0) return false;
        hipStream_t s = stream_.get();
        if (held_.size() == 1 && held_[0].rows == store_.rows) {
            // the one page of the input, still where its owner put it: its block arrays ARE the columns (released when the operator goes)
            for (size_t c = 0; c < types_.size(); c++) {
                if (!needed_[c]) continue;
                const pa_column& in = held_[0].cols[c];
                store_.cols[c].values.borrow(in.values, (size_t)store_.rows * type_width(types_[c]));
                if (in.nulls) {
                    store_.cols[c].nulls.borrow(in.nulls, (size_t)store_.rows);
                    store_.cols[c].has_nulls = true;
                }
            }
        }
        else flush_held();
        const int64_t n = store_.rows;
        // Output channels that can ride along with the pairs of the LAST sort (the first sort channel's) instead of being gathered by the
        // sorted row ids afterwards: flat 4- / 8-byte channels without NULL rows.  Whether they do is the sorter's to say (carry.moved: that
        // sort started from the identity permutation -- one sort channel, or the channels behind it all constant -- and the hand-written
        // sort took it).  payload_of[j] = its slot, or -1.
        const std::vector<int>& outs = output_channels_;
        std::vector<int> payload_of(outs.size(), -1);
        SortCarry carry;
        memset(&carry.payload, 0, sizeof carry.payload);
        const int first_channel = sort_channels_[0];
        const OutColumn& f = store_.cols[(size_t)first_channel];
        // (integers without NULL rows: the sorted images ARE the column)
        const bool images_serve = !f.varwidth && !f.has_nulls && (f.type == PA_BIGINT || f.type == PA_INTEGER || f.type == PA_DATE);
        if (!f.varwidth && !f.has_nulls && !getenv("PRESTO_AMD_SORT_NO_PAYLOAD")) {
            SortPayload& payload = carry.payload;
            for (size_t j = 0; j < outs.size() && payload.count < PA_SORT_MAX_PAYLOAD; j++) {
                const OutColumn& a = store_.cols[(size_t)outs[j]];
                const int w = a.varwidth ? 0 : type_width(a.type);
                if (a.has_nulls || (w != 4 && w != 8)) continue;
                if (outs[j] == first_channel && images_serve) continue;   // (written from the sorted images)
                payload_of[j] = payload.count;
                payload.in[payload.count] = a.values.ptr();
                payload.out[payload.count] = payload_out_[payload.count].ensure((size_t)n * w);
                payload.width[payload.count] = w;
                payload.count++;
            }
        }
        std::vector<DevColumn> sort_cols;
        for (int c : sort_channels_) sort_cols.push_back(store_.view(c));
        timer.begin(s);
        const int32_t* perm = sorter_.sort(sort_cols, sort_orders_, nullptr, 0, n, s, &carry);
        timer.end(s);
        // (pa_op_kernel_name: which sort the last image took)
        if (carry.path != PA_SORT_NONE) timer.set_name(carry.path == PA_SORT_LIBRARY ? "rocprim_radix_sort_pairs" : "pa_sort_buckets");
        // Output channels in sorted order (PagesIndex.appendTo).  Two kinds of channel are not gathered: one the sort brought along, and
        // the first sort channel as an output channel, when its sorted images serve and the sorter still has them.
        const uint64_t* sorted_images = images_serve ? carry.sorted_images : nullptr;
        out_cols_.clear();
        out_cols_.resize(outs.size());
        std::vector<bool> produced(outs.size(), false);
        for (size_t j = 0; j < outs.size(); j++) {
            const OutColumn& a = store_.cols[(size_t)outs[j]];
            if (a.varwidth) continue;
            if (carry.moved && payload_of[j] >= 0) out_cols_[j].values = std::move(payload_out_[payload_of[j]]);
            else if (sorted_images != nullptr && outs[j] == first_channel)
                launch_topn_values_of_keys(a.type, sorted_images, n, sort_orders_[0] >= 2, out_cols_[j].values.ensure((size_t)n * type_width(a.type)), s);
            else continue;
            produced[j] = true;
        }
        store_.gather_sorted(perm, n, outs, &produced, out_cols_, gather_, s);
        publish_output(out_cols_, (int32_t)n, output_mem_, s, out, out_storage_);
        return true;
    }

    int64_t memory_bytes() override
    {
        return (int64_t)(store_.bytes() + gather_.bytes());
    }

private:
    Stream stream_;
    PageStager stager_;
    std::vector<int32_t> types_, sort_orders_;
    std::vector<int> output_channels_, sort_channels_;
    std::vector<bool> needed_;
    HeldRows store_;   // (store_.rows counts the rows of the listed pages too)
    // device pages listed instead of copied (add_input)
    struct Held {
        int64_t rows = 0;
        std::vector<pa_column> cols;
        void (*release)(void*) = nullptr;
        void* release_ctx = nullptr;
    };
    std::vector<Held> held_;
    int32_t output_mem_ = PA_MEM_HOST;
    bool finishing_ = false, output_done_ = false;
    RowSorter sorter_;
    DevBuf payload_out_[PA_SORT_MAX_PAYLOAD];
    PositionGather gather_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> out_storage_;
};

}  // namespace

pa_operator* make_order_by(const pa_order_by_desc* desc)
{
    PA_REQUIRE(desc != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    return new OrderByOperator(desc);
}

}  // namespace pa
