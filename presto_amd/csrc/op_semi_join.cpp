// op_semi_join.cpp -- SetBuilderOperator + HashSemiJoinOperator (semi-join, `x [NOT] IN (SELECT y ...)`) on device.
//
// Reference path replaced:
//   LocalExecutionPlanner.visitSemiJoin (…/sql/planner/LocalExecutionPlanner.java:2749-2835)
//   SetBuilderOperator (…/operator/SetBuilderOperator.java) -> ChannelSet (…/operator/ChannelSet.java)
//   HashSemiJoinOperator (…/operator/HashSemiJoinOperator.java:168-221)
//
// Contract (include/presto_amd.h).  The probe's output page is its input page with one BOOLEAN column appended; for the probe key k
// of a row the mark is (HashSemiJoinOperator.java:190-218):
//   k NULL,     set without positions                 -> false
//   k NULL,     set with positions                    -> NULL
//   k not NULL, k in the set                          -> true
//   k not NULL, k not in the set, set holds a NULL    -> NULL
//   k not NULL, k not in the set, no NULL in the set  -> false
// Membership is the set's IS NOT DISTINCT FROM (ChannelSet.contains -> GroupByHash.contains -> positionNotDistinctFromRow): any NaN
// matches any NaN and -0.0 matches +0.0 (DoubleType.java:181-192), VARCHAR compares bytes, any non-zero BOOLEAN byte is true.
// "Empty" is zero build positions: a set of NULLs only is not empty (ChannelSet.isEmpty counts the NULL group).
//
// Build: the join build (op_join.cpp) into a lookup source over ONE key -- the canonical 64-bit form of the set value
// (semi_join_kernels.hpp) as a BIGINT for every type but VARCHAR, so NaN / -0.0 / BOOLEAN bytes compare right and the keyed layouts
// (bitmap, rank index, key slots) serve them all; VARCHAR goes through the generic tagged table.  $hashvalue channels are accepted
// and not read: the canonical key is hashed (a DOUBLE's $hashvalue need not agree for -0.0 and +0.0), so they change no result.
// Probe: one mark pass per page (semi_join_kernels.hip), one specialisation per layout; the output page, with the retained probe page
// behind it, is keyed_operator.hpp's PassThroughOutput.
#include "join_source.hpp"
#include "keyed_operator.hpp"
#include "semi_join_kernels.hpp"
#include "static_kernels.hpp"

namespace pa {

// SetBuilderOperator.SetSupplier: what the builder publishes and the probe operators read
struct ChannelSetImpl {
    std::atomic<bool> has_builder{false};
    std::atomic<int32_t> type{-1};          // the set channel's type, once a builder exists
    std::atomic<int32_t> type_param{0};     // ... and its PA_DECIMAL_PARAM (stored before `type`)
    std::shared_ptr<LookupSourceImpl> ls;   // the lookup source over the canonical key (null: no position)
    int64_t positions = 0;                  // build positions, NULL rows included
    bool contains_null = false;
    int32_t layout = SEMI_EMPTY;
    std::atomic<int32_t> error{0};          // the build failed (a pa_status): published with `built`, the probes raise it
    std::atomic<bool> built{false};         // set last, after everything above
    std::mutex mu;
    int64_t size = -1;                      // ChannelSet.size(), computed when first asked for
};

}  // namespace pa

struct pa_channel_set {
    std::shared_ptr<pa::ChannelSetImpl> impl;
};

namespace pa {
namespace {

// the descriptor checks come before the device: a shape the device path does not take is reported as such everywhere
void* checked_stream(const pa_set_builder_desc* d)
{
    PA_REQUIRE(d != nullptr && d->input_types != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    PA_REQUIRE(d->input_channel_count > 0 && d->input_channel_count <= 32, PA_ERR_NOT_SUPPORTED, "1..32 build channels");
    check_key_channels(&d->set_channel, 1, d->input_channel_count, d->input_types, "semi-join");
    check_hash_channel(d->hash_channel, d->input_channel_count, d->input_types);
    return d->stream;
}
void* checked_stream(const pa_hash_semi_join_desc* d)
{
    PA_REQUIRE(d != nullptr && d->probe_types != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    check_input_channels(d->probe_channel_count);
    check_key_channels(&d->probe_join_channel, 1, d->probe_channel_count, d->probe_types, "semi-join");
    check_hash_channel(d->probe_hash_channel, d->probe_channel_count, d->probe_types);
    check_output_mem(d->output_mem);
    return d->stream;
}

class SetBuilderOperator : public pa_operator {
public:
    SetBuilderOperator(const pa_set_builder_desc* d, pa_channel_set* set) : stream_(checked_stream(d))
    {
        PA_REQUIRE(set != nullptr && set->impl != nullptr, PA_ERR_INVALID_ARGUMENT, "set is null");
        key_type_ = d->input_types[d->set_channel];
        set_channel_ = d->set_channel;
        channels_ = d->input_channel_count;
        needed_.assign(channels_, false);
        needed_[set_channel_] = true;
        const int32_t inner_type = key_type_ == PA_VARCHAR ? PA_VARCHAR : PA_BIGINT;
        const int32_t zero = 0;
        pa_hash_builder_desc hd;
        memset(&hd, 0, sizeof hd);
        hd.input_channel_count = 1;
        hd.input_types = &inner_type;
        hd.join_channel_count = 1;
        hd.join_channels = &zero;
        hd.hash_channel = -1;
        hd.expected_positions = d->expected_positions;
        hd.stream = stream_.get();
        key_param_ = d->input_type_params ? d->input_type_params[d->set_channel] : 0;
        PA_REQUIRE(!set->impl->has_builder.load(), PA_ERR_ILLEGAL_STATE, "the set already has a builder");
        inner_.reset(make_hash_builder(&hd, &bridge_));
        flag_ = static_cast<int32_t*>(flag_buf_.ensure(64));
        PA_HIP(hipMemsetAsync(flag_, 0, 64, stream_.get()));
        // the set is claimed last: a builder whose creation failed above leaves it free for the next one
        PA_REQUIRE(!set->impl->has_builder.exchange(true), PA_ERR_ILLEGAL_STATE, "the set already has a builder");
        set_ = set->impl;
        set_->type_param.store(key_type_ == PA_DECIMAL ? key_param_ : 0);
        set_->type.store(key_type_);
    }
    ~SetBuilderOperator() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t main_stream() override { return stream_.get(); }
    KernelTimer& kernel_timer() override { return inner_->kernel_timer(); }

    bool needs_input() override { return !finishing_; }

    // SetBuilderOperator.addInput: the set channel's values (canonical keys) into the build
    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(!finishing_, PA_ERR_ILLEGAL_STATE, "Operator is already finishing");
        PA_REQUIRE(page != nullptr && page->channel_count == channels_, PA_ERR_INVALID_ARGUMENT, "page does not match the build types");
        const int32_t m = page->position_count;
        if (m <= 0) return;
        PA_REQUIRE(positions_ + m <= INT32_MAX, PA_ERR_INSUFFICIENT_RESOURCES, "set exceeds 2^31 positions");
        hipStream_t s = stream_.get();
        DevPage dp = stager_.stage(page, &needed_, s);
        const DevColumn& c = dp.cols[set_channel_];
        PA_REQUIRE(c.type == key_type_, PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared set type");
        pa_column col;
        memset(&col, 0, sizeof col);
        col.nulls = c.nulls;
        if (key_type_ == PA_VARCHAR) {
            launch_semi_any_null(c.nulls, m, flag_, s);
            col.type = PA_VARCHAR;
            col.encoding = PA_VARWIDTH;
            col.values = c.values;
            col.offsets = c.offsets;
        }
        else {
            JoinCol jc{c.values, nullptr, c.nulls, c.type, 0};
            uint64_t* canon = static_cast<uint64_t*>(canon_.ensure((size_t)m * 8));
            launch_semi_canon(jc, m, canon, flag_, s);
            col.type = PA_BIGINT;
            col.encoding = PA_FLAT;
            col.values = canon;
        }
        pa_page inner;
        memset(&inner, 0, sizeof inner);
        inner.position_count = m;
        inner.channel_count = 1;
        inner.columns = &col;
        inner.mem = PA_MEM_DEVICE;
        inner_->add_input(&inner);   // (copies into the build columns on this stream: canon_ is free again in stream order)
        positions_ += m;
        if (page->mem != PA_MEM_DEVICE) PA_HIP(hipStreamSynchronize(s));  // (the stager's arena is overwritten by the next page)
    }

    // finishInput: the lookup source, then the set is published
    void finish() override
    {
        if (finishing_) return;
        finishing_ = true;
        int32_t any_null = 0;
        ChannelSetImpl& set = *set_;
        if (positions_ > 0) {
            try {
                inner_->finish();
                read_back(&any_null, flag_, 4, stream_.get());
            }
            catch (const Error& e) {
                // (HashBuilderOperator publishes its error with `built`: so does the set -- its probes raise it instead of waiting)
                set.error.store(e.code);
                set.built.store(true);
                throw;
            }
        }
        set.positions = positions_;
        set.contains_null = any_null != 0;
        if (positions_ > 0) {
            set.ls = bridge_.impl;
            if (key_type_ == PA_VARCHAR) set.layout = SEMI_TAGGED;
            else set.layout = set.ls->bitmap.bits ? SEMI_BITMAP : SEMI_SLOTS;
        }
        set.built.store(true);
    }
    bool get_output(pa_page*) override { return false; }
    bool is_finished() override { return finishing_; }
    int64_t memory_bytes() override { return inner_->memory_bytes() + (int64_t)canon_.capacity(); }

private:
    Stream stream_;
    PageStager stager_;
    pa_lookup_source bridge_;
    std::unique_ptr<pa_operator> inner_;
    std::shared_ptr<ChannelSetImpl> set_;
    std::vector<bool> needed_;
    DevBuf canon_, flag_buf_;
    int32_t* flag_ = nullptr;
    int32_t key_type_ = PA_BIGINT, key_param_ = 0, set_channel_ = 0, channels_ = 0;
    int64_t positions_ = 0;
    bool finishing_ = false;
};

class HashSemiJoinOperator : public pa_operator {
public:
    HashSemiJoinOperator(const pa_hash_semi_join_desc* d, pa_channel_set* set) : stream_(checked_stream(d))
    {
        PA_REQUIRE(set != nullptr && set->impl != nullptr, PA_ERR_INVALID_ARGUMENT, "set is null");
        set_ = set->impl;
        types_.assign(d->probe_types, d->probe_types + d->probe_channel_count);
        key_channel_ = d->probe_join_channel;
        key_param_ = types_[key_channel_] == PA_DECIMAL && d->probe_type_params ? d->probe_type_params[key_channel_] : 0;
        check_key_type();
        pass_.init(types_.size(), all_channels(types_.size()), {key_channel_}, d->output_mem);
        flag_ = static_cast<int32_t*>(flag_buf_.ensure(64));
        h_flag_ = static_cast<int32_t*>(h_flag_buf_.ensure(64));
    }
    ~HashSemiJoinOperator() override
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
        if (set_->built.load() && set_->error.load() != 0) throw Error(set_->error.load(), "the set's build failed on device");
        return !finishing_ && !pending_ && set_->built.load();
    }
    bool is_blocked() override { return !set_->built.load(); }

    void add_input(const pa_page* page) override
    {
        pass_.release(stream_.get());
        pass_.hold(page);
        PA_REQUIRE(set_->built.load(), PA_ERR_ILLEGAL_STATE, "the set is not built yet");
        if (set_->error.load() != 0) throw Error(set_->error.load(), "the set's build failed on device");
        PA_REQUIRE(!finishing_ && !pending_, PA_ERR_ILLEGAL_STATE, "Operator does not need input");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)types_.size(), PA_ERR_INVALID_ARGUMENT, "probe page does not match the probe types");
        check_key_type();
        const int32_t n = page->position_count;
        if (n <= 0) return;   // (LookupJoinOperator: a zero-row page produces nothing)
        hipStream_t s = stream_.get();
        // Page.appendColumn: the input blocks as they are where they can stay (their encodings included), the mark behind them
        const DevColumn& key = pass_.stage(stager_, page, true, s).cols[key_channel_];
        PA_REQUIRE(key.type == types_[key_channel_], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared probe type");
        const ChannelSetImpl& set = *set_;
        SemiProbeArgs a;
        memset(&a, 0, sizeof a);
        a.key = JoinCol{key.values, key.offsets, key.nulls, key.type, 0};
        a.n = n;
        a.layout = set.layout;
        a.miss_is_null = set.contains_null ? 1 : 0;
        a.null_is_null = set.positions > 0 ? 1 : 0;
        const size_t padded = ((size_t)n + 3) & ~(size_t)3;
        a.mark = static_cast<uint8_t*>(mark_.ensure(padded));
        may_null_ = (key.nulls != nullptr && set.positions > 0) || set.contains_null;
        if (may_null_) {
            a.mark_null = static_cast<uint8_t*>(mark_null_.ensure(padded));
            a.any_null_mark = flag_;
            PA_HIP(hipMemsetAsync(flag_, 0, 4, s));
        }
        if (set.layout != SEMI_EMPTY) {
            const LookupSourceImpl& ls = *set.ls;
            a.bitmap = ls.bitmap;
            a.slots = ls.key_slots.as<JoinKeySlot>();
            a.mask = ls.probe_mask;
            a.wrap = ls.probe_wrap;
            if (set.layout == SEMI_TAGGED) {
                a.build_key = ls.build_keys().col[0];
                a.tagged = ls.tagged.as<uint64_t>();
                HashPageArgs ha;
                memset(&ha, 0, sizeof ha);
                ha.col[0].values = key.values;
                ha.col[0].offsets = key.offsets;
                ha.col[0].nulls = key.nulls;
                ha.col[0].type = key.type;
                ha.ncols = 1;
                ha.n = n;
                ha.out = static_cast<int64_t*>(hash_.ensure((size_t)n * 8));
                launch_hash_page(ha, s);
                a.probe_hash = ha.out;
            }
        }
        timer.begin(s);
        timer.set_name(launch_semi_mark(a, s));
        timer.end(s);
        if (may_null_) PA_HIP(hipMemcpyAsync(h_flag_, flag_, 4, hipMemcpyDeviceToHost, s));
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
        hipStream_t s = stream_.get();
        bool null_marks = false;
        if (may_null_) {
            PA_HIP(hipStreamSynchronize(s));
            null_marks = *h_flag_ != 0;
        }
        pass_.publish(n_, PA_BOOLEAN, mark_.ptr(), null_marks ? mark_null_.as<uint8_t>() : nullptr, s, out);
        return true;
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finishing_ && !pending_; }
    void close() override
    {
        (void)hipStreamSynchronize(stream_.get());
        pass_.release(stream_.get());
    }
    int64_t memory_bytes() override { return (int64_t)(stager_.bytes() + mark_.capacity() + mark_null_.capacity() + hash_.capacity()); }

private:
    // build and probe key types must be equal: a DECIMAL's precision and scale too (a VARCHAR(n) bound need not: bytes are compared)
    void check_key_type() const
    {
        const int32_t t = set_->type.load();
        if (t < 0) return;  // no builder yet: checked again with every page
        PA_REQUIRE(t == types_[key_channel_], PA_ERR_INVALID_ARGUMENT, "probe / set key types differ");
        PA_REQUIRE(t != PA_DECIMAL || set_->type_param.load() == key_param_, PA_ERR_INVALID_ARGUMENT, "probe / set DECIMAL precision or scale differ");
    }

    Stream stream_;
    PageStager stager_;
    std::shared_ptr<ChannelSetImpl> set_;
    std::vector<int32_t> types_;
    PassThroughOutput pass_;
    int32_t key_channel_ = 0, key_param_ = 0, n_ = 0;
    DevBuf mark_, mark_null_, hash_, flag_buf_;
    PinnedBuf h_flag_buf_;
    int32_t* flag_ = nullptr;
    int32_t* h_flag_ = nullptr;
    bool may_null_ = false, pending_ = false, finishing_ = false;
};

}  // namespace

pa_channel_set* channel_set_new()
{
    pa_channel_set* s = new pa_channel_set;
    s->impl = std::make_shared<ChannelSetImpl>();
    return s;
}
void channel_set_delete(pa_channel_set* set) { delete set; }

void channel_set_stats(pa_channel_set* set, int64_t* size, int32_t* contains_null)
{
    PA_REQUIRE(set != nullptr && set->impl != nullptr, PA_ERR_INVALID_ARGUMENT, "set is null");
    ChannelSetImpl& s = *set->impl;
    PA_REQUIRE(s.built.load(), PA_ERR_ILLEGAL_STATE, "the set is not built yet");
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.size < 0) {
        uint64_t distinct = 0;
        if (s.positions > 0) {
            Stream st(nullptr);
            DevBuf out;
            unsigned long long* d = static_cast<unsigned long long*>(out.ensure(64));
            PA_HIP(hipMemsetAsync(d, 0, 8, st.get()));
            const LookupSourceImpl& ls = *s.ls;
            if (s.layout == SEMI_BITMAP) launch_semi_count_bits(ls.bitmap.bits, (int64_t)(ls.bitmap.range >> 6) + 1, d, st.get());
            else if (s.layout == SEMI_SLOTS) launch_semi_count_slots(ls.key_slots.as<JoinKeySlot>(), (int64_t)ls.probe_mask + 1, d, st.get());
            else launch_semi_count_tagged(ls.tagged.as<uint64_t>(), (int64_t)ls.probe_mask + 1, d, st.get());
            read_back(&distinct, d, 8, st.get());
        }
        s.size = (int64_t)distinct + (s.contains_null ? 1 : 0);   // (the NULL group is one value of the set)
    }
    if (size) *size = s.size;
    if (contains_null) *contains_null = s.contains_null ? 1 : 0;
}

pa_operator* make_set_builder(const pa_set_builder_desc* desc, pa_channel_set* set) { return new SetBuilderOperator(desc, set); }
pa_operator* make_hash_semi_join(const pa_hash_semi_join_desc* desc, pa_channel_set* set) { return new HashSemiJoinOperator(desc, set); }

}  // namespace pa
