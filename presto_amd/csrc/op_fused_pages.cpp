// op_fused_pages.cpp -- FusedAggregationOperator (op_fused.hpp): what happens to a page before it is launched.  Retained pages (their
// releases travel with the structure the page went to), small pages (ranges of stable pages that continue each other, the two arenas
// the others are copied into) and the range tables that hand many stable ranges to one launch.
#include <algorithm>
#include <cstring>

#include "op_fused.hpp"

namespace pa {
namespace fused_op {

void FusedAggregationOperator::release_checkpoint(std::vector<Release> rel, bool needs_confirm)
{
    if (rel.empty()) return;
    ReleaseBatch b;
    if (release_events_.empty()) PA_HIP(hipEventCreateWithFlags(&b.event, hipEventDisableTiming));
    else {
        b.event = release_events_.back();
        release_events_.pop_back();
    }
    PA_HIP(hipEventRecord(b.event, stream_.get()));
    b.seq = needs_confirm ? lds_.launch_seq : 0;
    b.rel = std::move(rel);
    release_batches_.push_back(std::move(b));
}

void FusedAggregationOperator::poll_releases()
{
    while (!release_batches_.empty()) {
        ReleaseBatch& b = release_batches_.front();
        if (b.seq != 0 && !lds_.inflight.empty() && lds_.inflight.front().seq <= b.seq) break;
        if (hipEventQuery(b.event) != hipSuccess) {
            (void)hipGetLastError();  // hipErrorNotReady is not an error here
            break;
        }
        for (const Release& r : b.rel) r.fn(r.ctx);
        release_events_.push_back(b.event);
        release_batches_.pop_front();
    }
}

// every release the operator still owes, now: the caller has made sure nothing reads the pages any more (stream drained)
void FusedAggregationOperator::release_everything()
{
    for (ReleaseBatch& b : release_batches_) {
        for (const Release& r : b.rel) r.fn(r.ctx);
        release_events_.push_back(b.event);
    }
    release_batches_.clear();
    auto fire = [](std::vector<Release>& v) {
        for (const Release& r : v) r.fn(r.ctx);
        v.clear();
    };
    fire(run_rel_);
    fire(ranges_rel_);
    fire(carry_rel_);
    fire(arena_[0].rel);
    fire(arena_[1].rel);
    if (cur_rel_set_) {
        cur_rel_set_ = false;
        cur_rel_.fn(cur_rel_.ctx);
    }
}

int64_t FusedAggregationOperator::gather_rows()
{
    const char* e = getenv("PRESTO_AMD_GATHER_ROWS");  // tests and sweeps move the launch threshold
    return e ? std::max<int64_t>(strtoll(e, nullptr, 10), 1) : (int64_t)1 << 26;
}

// true: the page was taken (merged into the pending range / copied into the arena)
bool FusedAggregationOperator::gather_small_page(const pa_page* page)
{
    const int64_t n = page->position_count;
    const bool stable_dev = page_stays(page) && page->mem == PA_MEM_DEVICE;
    if (run_.rows > 0) {
        // does the page continue the pending range?
        bool cont = stable_dev && run_.rows + n <= ((int64_t)1 << 30);
        for (int c = 0; c < spec_.n_in && cont; c++) {
            if (!spec_.used_channel[c]) continue;
            const pa_column& a = run_.cols[c];
            const pa_column& b = page->columns[c];
            cont = a.encoding == b.encoding && a.type == b.type && (a.nulls == nullptr) == (b.nulls == nullptr);
            if (!cont) break;
            if (a.nulls) cont = b.nulls == a.nulls + run_.rows;
            if (a.encoding == PA_FLAT) {
                cont = cont && b.values == static_cast<const char*>(a.values) + run_.rows * type_width(a.type);
            }
            else {
                cont = cont && b.values == a.values && b.offsets == a.offsets + run_.rows;
            }
        }
        if (cont) {
            run_.rows += n;
            if (cur_rel_set_) run_rel_.push_back(take_cur_release());
            if (run_.rows >= gather_rows()) flush_pending();
            return true;
        }
        retire_run();
        if (next_) return false;  // (add_input hands the page to the generation a flush started)
    }
    bool plain = true, flat = true;
    for (int c = 0; c < spec_.n_in && plain; c++) {
        if (!spec_.used_channel[c]) continue;
        plain = channel_plain(page->columns[c], c) && !spec_.derived(c);
        flat = flat && page->columns[c].encoding == PA_FLAT;
    }
    if (!plain) return false;
    if (stable_dev && n < gather_rows()) {
        // a range starts here: whatever its size, the next page may continue it
        run_.rows = n;
        run_.flat = flat;
        run_.cols.assign(page->columns, page->columns + page->channel_count);
        if (cur_rel_set_) run_rel_.push_back(take_cur_release());
        return true;
    }
    if (n >= kSmallPageRows) return false;
    // VariableWidthBlocks join the arena too: the bytes are appended and the offsets rebased on the way -- by the host's
    // arithmetic when the offsets can be read here (host pages), by a byte cursor in HBM for device pages, whose first
    // offset and byte count only the device knows (launch_var_append)
    if (!flat && page->mem != PA_MEM_HOST && !device_var_gatherable()) return false;
    append_to_arena(page);
    return true;
}

// A device page's VariableWidthBlocks are appended without the host knowing how many bytes they hold: the arena's byte
// buffers are sized for the most the declared types allow -- VARCHAR(n), n code points of at most 4 bytes -- which is kept
// to 64 bytes per row (n <= 16); unbounded or longer channels get a launch per page as before.
bool FusedAggregationOperator::device_var_gatherable() const
{
    int slots = 0;
    for (int c = 0; c < spec_.n_in; c++) {
        if (!spec_.used_channel[c] || spec_.in_types[c] != PA_VARCHAR) continue;
        if (spec_.in_params[c] < 1 || spec_.in_params[c] > kDeviceVarMaxLength) return false;
        slots++;
    }
    return slots <= kInlineVarSegs;
}

// The pending range ends (the next page does not continue it): a small one joins the arena -- one segment-copy launch --
// instead of getting a fused launch and its merges of its own; a large one is launched as it is.
void FusedAggregationOperator::retire_run()
{
    if (run_.rows == 0) return;
    if (run_.rows < kRangeTableRows && ranges_possible()) {
        // the ungrouped / few-groups kernels take such ranges in place, as a table: no copy at all.  (The first launch of
        // the few-groups tier decides whether it is the right one: nothing is collected before it is confirmed)
        if (mode_ == V_LDS && !lds_.probed) {
            flush_run();
            return;
        }
        DevPage r;
        r.n = (int32_t)run_.rows;
        r.cols.resize((size_t)spec_.n_in);
        for (int c = 0; c < spec_.n_in; c++) {
            if (!spec_.used_channel[c]) continue;
            const pa_column& col = run_.cols[c];
            r.cols[c].type = col.type;
            r.cols[c].varwidth = col.encoding == PA_VARWIDTH;
            r.cols[c].values = col.values;
            r.cols[c].offsets = col.offsets;
            r.cols[c].nulls = col.nulls;
        }
        if (!ranges_) ranges_ = std::make_shared<std::vector<DevPage>>();
        ranges_->push_back(std::move(r));
        range_rows_ += run_.rows;
        run_.rows = 0;
        ranges_rel_.insert(ranges_rel_.end(), run_rel_.begin(), run_rel_.end());
        run_rel_.clear();
        if (range_rows_ >= std::min<int64_t>(gather_rows(), (int64_t)1 << 30) || ranges_->size() >= kMaxRanges) flush_ranges();
        return;
    }
    if (run_.rows >= kSmallPageRows || (!run_.flat && !device_var_gatherable())) {
        flush_run();
        return;
    }
    pa_page sp{};
    sp.position_count = (int32_t)run_.rows;
    sp.channel_count = spec_.n_in;
    sp.columns = run_.cols.data();
    sp.mem = PA_MEM_DEVICE;
    sp.flags = PA_PAGE_STABLE;  // its copy can wait for the arena's launch
    run_.rows = 0;
    carry_rel_.insert(carry_rel_.end(), run_rel_.begin(), run_rel_.end());  // the releases of the run's pages go where its rows go
    run_rel_.clear();
    append_to_arena(&sp);
}

// stable device ranges can be handed over as a table when the tier in charge has a kernel for it
bool FusedAggregationOperator::ranges_possible() const
{
    if (spec_.join || getenv("PRESTO_AMD_NO_RANGES")) return false;
    if (mode_ != V_GLOBAL && mode_ != V_LDS) return false;
    for (int c = 0; c < spec_.n_in; c++) {
        if (spec_.used_channel[c] && spec_.derived(c)) return false;
    }
    return true;
}

void FusedAggregationOperator::flush_ranges()
{
    if (!ranges_ || ranges_->empty()) return;
    std::shared_ptr<const std::vector<DevPage>> set = std::move(ranges_);
    ranges_.reset();
    const int64_t rows = range_rows_;
    range_rows_ = 0;
    std::vector<Release> rel;
    rel.swap(ranges_rel_);
    const uint64_t launched = timer.begun();
    try {
        process_ranges(set, rows);
    }
    catch (const PoolExhausted&) {
        // nothing of the table was launched: it waits with the page that is being parked (take_page)
        if (timer.begun() == launched && !next_) {
            ranges_ = std::make_shared<std::vector<DevPage>>(*set);
            range_rows_ = rows;
            ranges_rel_.swap(rel);
        }
        else release_checkpoint(std::move(rel), true);
        throw;
    }
    release_checkpoint(std::move(rel), true);
}

void FusedAggregationOperator::process_ranges(const std::shared_ptr<const std::vector<DevPage>>& set, int64_t rows)
{
    if (next_) {
        next_->process_ranges(set, rows);
        return;
    }
    retained_ = true;
    try {
        DevPage dp;
        dp.n = (int32_t)rows;
        dp.cols = set->front().cols;
        dp.ranges = set;
        std::vector<ChannelLayout> layout(spec_.n_in);
        std::string sig;
        for (int c = 0; c < spec_.n_in; c++) {
            layout[c].type = spec_.in_types[c];
            if (spec_.used_channel[c]) {
                for (const DevPage& r : *set) {
                    PA_REQUIRE(r.cols[c].type == spec_.in_types[c], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared input type");
                    if (r.cols[c].nulls != nullptr) nullable_seen_[c] = true;
                }
            }
            layout[c].nullable = nullable_seen_[c];
            sig += layout[c].nullable ? 'n' : '-';
        }
        run_tiers(sig, layout, dp, true, 0);
    }
    catch (const LayoutChange&) {
        start_next_generation();
        next_->process_ranges(set, rows);
    }
    retained_ = false;
}

bool FusedAggregationOperator::range_aligned(const DevPage& r, const std::vector<bool>& used)
{
    bool vec = true;
    for (size_t c = 0; c < r.cols.size(); c++) {
        if (!used[c]) continue;
        vec = vec && ((uintptr_t)r.cols[c].values % 16 == 0) && ((uintptr_t)r.cols[c].offsets % 16 == 0) && ((uintptr_t)r.cols[c].nulls % 4 == 0);
    }
    return vec;
}

void FusedAggregationOperator::flush_run()
{
    if (run_.rows == 0) return;
    pa_page sp{};
    sp.position_count = (int32_t)run_.rows;
    sp.channel_count = spec_.n_in;
    sp.columns = run_.cols.data();
    sp.mem = PA_MEM_DEVICE;
    sp.flags = PA_PAGE_STABLE;
    run_.rows = 0;
    std::vector<pa_column> cols;
    cols.swap(run_.cols);  // (process_page may come back here through a generation change)
    sp.columns = cols.data();
    std::vector<Release> rel;
    rel.swap(run_rel_);
    try {
        process_page(&sp, true);
    }
    catch (...) {
        release_checkpoint(std::move(rel), true);  // (whatever of the range was launched is in the stream in front of the event)
        throw;
    }
    release_checkpoint(std::move(rel), true);
}

void FusedAggregationOperator::append_to_arena(const pa_page* page)
{
    hipStream_t s = stream_.get();
    const int64_t n = page->position_count;
    Arena& a = arena_[arena_cur_];
    // the nullability of the arena's channels is fixed by its first page: a page that differs starts the next arena
    bool fits = a.rows + n <= kArenaRows && a.segs.size() + 3 * (size_t)spec_.n_in <= kArenaMaxSegs && a.vsegs.size() + (size_t)spec_.n_in <= kArenaMaxSegs;
    // the byte cursor of a VARCHAR channel is either the host's (a.bytes) or the device's: pages of the other kind start the next arena
    const bool dev_var = page->mem != PA_MEM_HOST;
    for (int c = 0; c < spec_.n_in && fits && a.rows > 0; c++) {
        if (!spec_.used_channel[c]) continue;
        const pa_column& col = page->columns[c];
        fits = a.nullable[c] == (col.nulls != nullptr);
        if (fits && col.encoding == PA_VARWIDTH) fits = a.dev_var == dev_var;
        // a VARCHAR channel's byte buffer never moves while copies into it are pending
        if (fits && col.encoding == PA_VARWIDTH && col.offsets != nullptr && !dev_var) {
            fits = a.bytes[c] + ((int64_t)col.offsets[n] - col.offsets[0]) <= (int64_t)a.values[c].capacity();
        }
    }
    if (!fits) {
        flush_pending();
        if (next_) {  // the flush started the next generation
            std::vector<Release> carried;
            carried.swap(carry_rel_);
            // the page itself: the generation registers its release (it sees the flag); a gathered run's releases cannot travel
            // through add_input -- they are called once the generation has launched and confirmed the run's rows
            if (cur_rel_set_ && (page->flags & PA_PAGE_RETAINED) != 0 && page->release == cur_rel_.fn && page->release_ctx == cur_rel_.ctx) cur_rel_set_ = false;
            next_->add_input(page);
            if (!carried.empty()) {
                next_->flush_pending();
                next_->confirm_all();
                release_checkpoint(std::move(carried), false);
            }
            return;
        }
        return append_to_arena(page);
    }
    // a pageable host page: its arrays go behind each other into pinned memory, and ONE launch reads them from there (a copy per
    // array is ~4 us of enqueueing each)
    bool pinned_copy = false;
    if (page->mem == PA_MEM_HOST && (page->flags & PA_PAGE_PINNED) == 0) {
        if (const pa_page* pinned = pinned_copy_.copy(page, &spec_.used_channel)) {
            page = pinned;
            pinned_copy = true;
        }
    }
    const bool host = page->mem == PA_MEM_HOST;
    const bool readable = !host || (page->flags & PA_PAGE_PINNED) != 0;  // the device can read the page's buffers itself
    const bool defer = readable && page_stays(page);                       // ... and they stay: copy at the arena's launch
    if (cur_rel_set_) a.rel.push_back(take_cur_release());
    a.rel.insert(a.rel.end(), carry_rel_.begin(), carry_rel_.end());
    carry_rel_.clear();
    if (a.rows == 0) {
        a.nullable.assign(spec_.n_in, false);
        a.values.resize(spec_.n_in);
        a.nulls.resize(spec_.n_in);
        a.offsets.resize(spec_.n_in);
        a.bytes.assign(spec_.n_in, 0);
        a.dev_var = dev_var;
        a.var_fresh = true;
        for (int c = 0; c < spec_.n_in; c++) {
            if (!spec_.used_channel[c]) continue;
            a.nullable[c] = page->columns[c].nulls != nullptr;
            if (spec_.in_types[c] != PA_VARCHAR) a.values[c].ensure((size_t)kArenaRows * type_width(spec_.in_types[c]));
            if (a.nullable[c]) a.nulls[c].ensure((size_t)kArenaRows);
        }
    }
    CopySeg now[3 * PA_MAX_CHANNELS];
    VarSeg vnow[kInlineVarSegs];
    int m = 0, vm = 0, slot = 0;
    // the device cursors of this append: read from one half of a.cursors, left in the other (deferred appends of one
    // arena launch are planned together: launch_var_append takes the first one's input and the last one's output)
    int64_t* cur_in = nullptr;
    int64_t* cur_out = nullptr;
    if (dev_var) {
        int64_t* cursors = static_cast<int64_t*>(a.cursors.ensure(2 * kVarSlots * sizeof(int64_t)));
        const bool pending = defer && !a.vsegs.empty();  // a deferred append continues the pending plan: same halves
        if (!pending) a.cursor_half ^= 1;
        cur_in = cursors + (a.cursor_half ^ 1) * kVarSlots;
        cur_out = cursors + a.cursor_half * kVarSlots;
    }
    auto seg = [&](const void* src, void* dst, int64_t bytes, int32_t add = 0) {
        CopySeg sg{src, dst, bytes, 0};
        sg.add_i32 = add;
        if (defer) a.segs.push_back(sg);
        else now[m++] = sg;
    };
    for (int c = 0; c < spec_.n_in; c++) {
        if (!spec_.used_channel[c]) continue;
        const pa_column& col = page->columns[c];
        PA_REQUIRE(col.type == spec_.in_types[c], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared input type");
        PA_REQUIRE(col.values != nullptr, PA_ERR_INVALID_ARGUMENT, "block values is null");
        if (col.nulls) {
            char* dn = a.nulls[c].as<char>() + a.rows;
            if (readable) seg(col.nulls, dn, n);
            else PA_HIP(hipMemcpyAsync(dn, col.nulls, (size_t)n, hipMemcpyHostToDevice, s));
        }
        if (col.encoding == PA_VARWIDTH && dev_var) {
            // device page: where the block's bytes start and how many there are is only known over there
            PA_REQUIRE(col.offsets != nullptr, PA_ERR_INVALID_ARGUMENT, "VARWIDTH block without offsets");
            const int64_t row_bytes = 4 * (int64_t)spec_.in_params[c];
            if (a.rows == 0) a.values[c].ensure((size_t)(row_bytes * kArenaRows));
            VarSeg vs{};
            vs.values = static_cast<const char*>(col.values);
            vs.offsets = col.offsets;
            vs.dst_bytes = a.values[c].as<char>();
            vs.capacity = std::min<int64_t>((int64_t)a.values[c].capacity(), ((int64_t)1 << 31) - 1);
            vs.dst_offsets = static_cast<int32_t*>(a.offsets[c].ensure((size_t)(kArenaRows + 1) * 4)) + a.rows;
            vs.cursor_in = cur_in + slot;
            vs.cursor_out = cur_out + slot;
            vs.rows = (int32_t)n;
            vs.byte_wgs = (int32_t)std::min<int64_t>(std::max<int64_t>(n * std::min<int64_t>(row_bytes, 16) >> 16, 1), 64);
            vs.slot = slot++;
            vs.fresh = a.var_fresh ? 1 : 0;
            if (defer) a.vsegs.push_back(vs);
            else vnow[vm++] = vs;
            continue;
        }
        if (col.encoding == PA_VARWIDTH) {
            // host page: the offsets are readable here.  bytes behind the arena's bytes, offsets rebased by (cursor - first)
            PA_REQUIRE(col.offsets != nullptr, PA_ERR_INVALID_ARGUMENT, "VARWIDTH block without offsets");
            const int64_t first = col.offsets[0], len = (int64_t)col.offsets[n] - first;
            PA_REQUIRE(len >= 0 && a.bytes[c] + len < ((int64_t)1 << 31), PA_ERR_INVALID_ARGUMENT, "bad VARWIDTH offsets");
            int32_t* doff = static_cast<int32_t*>(a.offsets[c].ensure((size_t)(kArenaRows + 1) * 4)) + a.rows;
            if (a.rows == 0) {
                // sized by the channel's declared bound (VARCHAR(n)), or for this page with room to spare; a later page
                // that does not fit starts the next arena (see `fits`)
                const int64_t bound = spec_.in_params[c] > 0 ? std::min<int64_t>(spec_.in_params[c], 64) : 0;
                a.values[c].ensure((size_t)std::max<int64_t>({bound * kArenaRows, 4 * len, (int64_t)1 << 20}));
            }
            char* dv = a.values[c].as<char>() + a.bytes[c];
            const int32_t delta = (int32_t)(a.bytes[c] - first);
            if (readable) {
                seg(static_cast<const char*>(col.values) + first, dv, len);
                // (n + 1 entries: the first one rewrites the previous page's end with the same value)
                if (delta != 0) seg(col.offsets, doff, (n + 1) * 4, delta);
                else seg(col.offsets, doff, (n + 1) * 4);
            }
            else {
                if (len) PA_HIP(hipMemcpyAsync(dv, static_cast<const char*>(col.values) + first, (size_t)len, hipMemcpyHostToDevice, s));
                PA_HIP(hipMemcpyAsync(doff, col.offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
                if (delta != 0) {
                    CopySeg sg{doff, doff, (n + 1) * 4, 0};
                    sg.add_i32 = delta;
                    now[m++] = sg;  // in place, behind the copy in stream order
                }
            }
            a.bytes[c] += len;
            continue;
        }
        const int w = type_width(col.type);
        char* dv = a.values[c].as<char>() + a.rows * w;
        if (readable) seg(col.values, dv, n * w);
        else PA_HIP(hipMemcpyAsync(dv, col.values, (size_t)n * w, hipMemcpyHostToDevice, s));
    }
    if (m > 0) launch_copy_segments_inline(now, m, s);
    if (pinned_copy) pinned_copy_.used(s);
    if (vm > 0) {
        // (deferred appends recorded before this page come first: the cursor passes through them)
        flush_var_segments(a);
        launch_var_append_inline(vnow, vm, ctl_, s);
    }
    if (slot > 0) a.var_fresh = false;
    a.rows += n;
    if (a.rows >= kArenaRows) flush_pending();
}

// launches whatever is pending: the merged range of stable pages and the current arena
void FusedAggregationOperator::flush_pending()
{
    if (next_) next_->flush_pending();
    // a small pending range joins the table of the others; alone, it is launched in place as it is
    if (ranges_ && !ranges_->empty() && run_.rows > 0 && run_.rows < kRangeTableRows && ranges_possible()) retire_run();
    flush_ranges();
    flush_arena();
    flush_run();
}

// the deferred VariableWidthBlock appends of an arena: one planning launch and one copy launch for all of them
void FusedAggregationOperator::flush_var_segments(Arena& a)
{
    if (a.vsegs.empty()) return;
    hipStream_t s = stream_.get();
    if (a.vtable_used) PA_HIP(hipEventSynchronize(a.vtable_event));
    else PA_HIP(hipEventCreateWithFlags(&a.vtable_event, hipEventDisableTiming));
    a.vtable_used = true;
    launch_var_append(a.vsegs.data(), a.vsegs.size(), a.h_vtable.ensure(copy_var_table_bytes(a.vsegs.size())),
                      a.d_vtable.ensure(copy_var_table_bytes(a.vsegs.size())), ctl_, s);
    PA_HIP(hipEventRecord(a.vtable_event, s));
    a.vsegs.clear();
}

void FusedAggregationOperator::flush_arena()
{
    Arena& a = arena_[arena_cur_];
    if (a.rows == 0) return;
    hipStream_t s = stream_.get();
    if (!a.segs.empty()) {
        // the copies of the stable pages gathered in this arena, in one launch.  The staging table is written by the host:
        // the copy of its previous use must have left it
        if (a.table_used) PA_HIP(hipEventSynchronize(a.table_event));
        else PA_HIP(hipEventCreateWithFlags(&a.table_event, hipEventDisableTiming));
        a.table_used = true;
        launch_copy_segments(a.segs.data(), a.segs.size(), a.h_table.ensure(copy_segments_table_bytes(a.segs.size())),
                             a.d_table.ensure(copy_segments_table_bytes(a.segs.size())), s);
        PA_HIP(hipEventRecord(a.table_event, s));
        a.segs.clear();
    }
    flush_var_segments(a);
    {
        // the arena holds copies: the pages it was filled from are free once the copies in the stream have run
        std::vector<Release> rel;
        rel.swap(a.rel);
        release_checkpoint(std::move(rel), false);
    }
    std::vector<pa_column> cols((size_t)spec_.n_in);
    for (int c = 0; c < spec_.n_in; c++) {
        cols[c].type = spec_.in_types[c];
        cols[c].encoding = spec_.in_types[c] == PA_VARCHAR ? PA_VARWIDTH : PA_FLAT;
        if (!spec_.used_channel[c]) continue;
        cols[c].values = a.values[c].ptr();
        cols[c].offsets = spec_.in_types[c] == PA_VARCHAR ? a.offsets[c].as<int32_t>() : nullptr;
        cols[c].nulls = a.nullable[c] ? a.nulls[c].as<uint8_t>() : nullptr;
    }
    pa_page sp{};
    sp.position_count = (int32_t)a.rows;
    sp.channel_count = spec_.n_in;
    sp.columns = cols.data();
    sp.mem = PA_MEM_DEVICE;
    // VARCHAR channels gathered from host pages: the host placed the bytes, so it knows how many there are (StringInterner::intern)
    struct HintScope {
        std::vector<int64_t>& hint;
        ~HintScope() { hint.clear(); }
    } hint_scope{var_bytes_hint_};
    if (!a.dev_var) var_bytes_hint_.assign(a.bytes.begin(), a.bytes.end());
    a.rows = 0;
    arena_cur_ ^= 1;
    // the arena is this operator's own: its rows stay put until the launches on it are confirmed -- the other arena
    // takes the next pages, and is only written again after this one's launches were confirmed (kMaxInflight = 2)
    process_page(&sp, true);
}

// The table of a ranged launch (entry layout: range_entry_words): every range cut into entries of at most kRangeRows rows,
// each with its own buffer addresses.  Returns the number of entries.
int64_t FusedAggregationOperator::fill_range_table(const KernelInfo& ki, const DevPage& dp, PaFusedArgs& a, hipStream_t s)
{
    const std::vector<ChannelLayout>& layout = *cur_layout_;
    const int rw = range_entry_words(spec_, layout);
    const int64_t per = ki.variant == V_LDS ? kRangeRowsLds : kRangeRows;
    int64_t entries = 0;
    for (const DevPage& r : *dp.ranges) entries += (r.n + per - 1) / per;
    RangeTable& t = range_table_[range_table_next_];
    range_table_next_ = (range_table_next_ + 1) % 3;
    // the staging table is written by the host: the copy of its previous use must have left it
    if (t.used) PA_HIP(hipEventSynchronize(t.event));
    else PA_HIP(hipEventCreateWithFlags(&t.event, hipEventDisableTiming));
    t.used = true;
    const size_t bytes = (size_t)entries * rw * 8;
    uint64_t* w = static_cast<uint64_t*>(t.host.ensure(bytes));
    for (const DevPage& r : *dp.ranges) {
        const uint64_t vec = range_aligned(r, spec_.used_channel) ? 1 : 0;
        for (int64_t row0 = 0; row0 < r.n; row0 += per) {
            const int64_t n = std::min<int64_t>(per, r.n - row0);
            for (int c = 0; c < spec_.n_in; c++) {
                if (!spec_.used_channel[c]) continue;
                const DevColumn& col = r.cols[c];
                if (layout[c].type == PA_VARCHAR) {
                    *w++ = (uint64_t)(uintptr_t)col.values;
                    *w++ = (uint64_t)(uintptr_t)(col.offsets + row0);
                }
                else {
                    *w++ = (uint64_t)(uintptr_t)(static_cast<const char*>(col.values) + row0 * type_width(col.type));
                }
                if (layout[c].nullable) *w++ = col.nulls ? (uint64_t)(uintptr_t)(col.nulls + row0) : 0;
            }
            *w++ = (uint64_t)n | (vec << 32);
        }
    }
    void* dev = t.dev.ensure(bytes);
    PA_HIP(hipMemcpyAsync(dev, t.host.ptr(), bytes, hipMemcpyHostToDevice, s));
    PA_HIP(hipEventRecord(t.event, s));
    a.ranges = static_cast<const uint64_t*>(dev);
    a.n_ranges = entries;
    return entries;
}

}  // namespace fused_op
}  // namespace pa
