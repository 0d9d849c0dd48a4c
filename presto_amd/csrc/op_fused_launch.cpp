// op_fused_launch.cpp -- FusedAggregationOperator (op_fused.hpp): a staged page through the kernels.  add_page and run_tiers choose
// the tier (its code comes from op_fused_kernels.cpp), run_page fills the arguments every tier's kernel takes and hands over to one
// launcher per family of tiers -- launch_global (no groups), launch_lds (few groups, confirmed late: poll_inflight / confirm_*),
// launch_table (the HBM table and the LDS tables in front of it), run_page_build_rows (probe stage: the group is the build row).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "op_fused.hpp"

namespace pa {
namespace fused_op {

void FusedAggregationOperator::add_page(const pa_page* page)
{
    HostTraceScope trace("  fused.add_page");
    hipStream_t s = stream_.get();
    // interned key channels that arrive as a DictionaryBlock / RLE over strings take the dictionary route: not decoded
    std::vector<int> dict_keys;
    std::vector<bool> needed = spec_.used_channel;
    for (int c = 0; c < spec_.n_in; c++) {
        if (!spec_.interned[c]) continue;
        const pa_column& col = page->columns[c];
        const bool encoded = (col.encoding == PA_DICTIONARY && col.ids != nullptr) || col.encoding == PA_RLE;
        if (!encoded || col.dictionary == nullptr || col.dictionary->encoding != PA_VARWIDTH) continue;
        const int64_t dn = col.encoding == PA_RLE ? 1 : col.dictionary_size;
        if (dn <= 0 || dn > page->position_count) continue;
        needed[c] = false;
        dict_keys.push_back(c);
    }
    if (spec_.join && !join_checked_) {
        spec_.join->require_built();
        join_checked_ = true;
        // the group is the build row whenever the plan allows it: no hashing, no key compares, no spills
        if (grouped_ && !spec_.join->brow_group_proj.empty() && !getenv("PRESTO_AMD_NO_BROW")) mode_ = V_BROW;
    }
    DevPage dp = stager_.stage(page, &needed, s);
    for (int c : dict_keys) intern_dictionary_key(page, c, dp, s);
    intern_keys(dp, s);
    rank_values(dp, s);
    // layout signature of this page
    std::vector<ChannelLayout> layout(spec_.n_in);
    std::string sig;
    bool vec = true;
    for (int c = 0; c < spec_.n_in; c++) {
        layout[c].type = spec_.used_channel[c] ? dp.cols[c].type : spec_.in_types[c];
        // nullability only ever grows: a page without NULLs on a channel that had some runs the nullable kernels with a
        // null valueIsNull pointer, so the state layout changes at most once per channel
        if (spec_.used_channel[c] && dp.cols[c].nulls != nullptr) nullable_seen_[c] = true;
        layout[c].nullable = nullable_seen_[c];
        if (spec_.used_channel[c]) {
            PA_REQUIRE(dp.cols[c].type == spec_.in_types[c], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared input type");
            vec = vec && ((uintptr_t)dp.cols[c].values % 16 == 0) && ((uintptr_t)dp.cols[c].offsets % 16 == 0) &&
                  ((uintptr_t)dp.cols[c].nulls % 4 == 0);
        }
        sig += layout[c].nullable ? 'n' : '-';
    }
    if (spec_.join) spec_.join->append_build_channels(&layout, &sig);
    run_tiers(sig, layout, dp, vec, 0);
}

// rows [start_row, dp.n) of a staged page through the tier mode_ names, moving on to the next tier when it gives up
void FusedAggregationOperator::run_tiers(const std::string& sig, const std::vector<ChannelLayout>& layout, const DevPage& dp, bool vec, int64_t start_row)
{
    for (;;) {
        // launches of the few-groups variant still unconfirmed while another tier takes over: settle them first (their
        // merges write the table the other tiers resize and replicate)
        if (mode_ != V_LDS && !lds_.inflight.empty()) confirm_all();
        if (dp.ranges && mode_ != V_GLOBAL && mode_ != V_LDS) {
            // a table of ranges and a tier without a kernel for tables (the few-groups tier gave up): range by range
            for (const DevPage& r : *dp.ranges) run_tiers(sig, layout, r, range_aligned(r, spec_.used_channel), 0);
            break;
        }
        int partitions = 0;
        if (mode_ == V_GT && partitioned_wanted(sig, layout, &partitions)) {
            run_page_partitioned(sig, layout, dp, vec, partitions, start_row);
            break;
        }
        const Compiled* compiled = nullptr;
        try {
            if (mode_ == V_GLOBAL && !dp.ranges) compiled = staged_kernel(sig, layout, dp.n - start_row);
            if (!compiled) compiled = &kernel_for(sig, layout, dp.ranges ? (mode_ == V_GLOBAL ? V_GLOBAL_R : V_LDS_R) : mode_);
        }
        catch (const Error& e) {
            // the group state may be too wide for the wave's / the workgroup's LDS budget: move on to the next tier
            // (anything else that is not supported fails again there and surfaces)
            if (e.code != PA_ERR_NOT_SUPPORTED || (mode_ != V_LDS && mode_ != V_LDSH)) throw;
            mode_ = mode_ == V_LDS ? V_LDSH : V_GT;
            continue;
        }
        const Compiled& ck = *compiled;
        resume_from_ = -1;
        cur_sig_ = &sig;
        cur_layout_ = &layout;
        if (run_page(ck, dp, vec, nullptr, start_row)) break;
        if (resume_from_ >= 0) {
            // the rows before resume_from_ are done (or launched and waiting for their confirmation); the rest of the page
            // goes to the tier mode_ now names
            start_row = resume_from_;
            if (start_row >= dp.n) break;
            continue;
        }
        // the page held more groups than the wave's register table: redo it (and every later page) with the
        // workgroup-level LDS table, which itself hands rows it has no room for to the HBM table
        mode_ = V_LDSH;
    }
}

// BROW: accumulators indexed by build position.  The table has one slot per build row -- it never fills, nothing spills,
// nothing needs confirming: launches are enqueued and forgotten (the error word is read at finish).
bool FusedAggregationOperator::run_page_build_rows(const Compiled& ck, const DevPage& dp, PaFusedArgs a, int64_t start_row)
{
    HostTraceScope trace("    fused.run_page_build_rows");
    hipStream_t s = stream_.get();
    const KernelInfo& ki = ck.info;
    const uint32_t slots = (uint32_t)std::max(spec_.join->ls->n(), 1);
    if (gt_.cap == 0) {
        brow_occ_word_ = ki.occ_word;
        brow_occ_empty_ = ki.occ_empty;
        gt_.keys.ensure((size_t)slots * 8 * std::max(w_, 1));
        gt_.words.ensure((size_t)slots * 8 * nw_);
        gt_.rep_count.ensure(128 * 4);
        PA_HIP(hipMemsetAsync(gt_.words.ptr(), 0, (size_t)slots * 8 * nw_, s));
        if (brow_occ_word_ < 0) {
            gt_.tag.ensure((size_t)slots * 8);
            PA_HIP(hipMemsetAsync(gt_.tag.ptr(), 0, (size_t)slots * 8, s));
        }
        else if (brow_occ_empty_ != 0) {
            launch_fill_u64(gt_.words.as<uint64_t>() + (size_t)brow_occ_word_ * slots, brow_occ_empty_, (int64_t)slots, s);
        }
        PA_HIP(hipMemsetAsync(gt_.rep_count.ptr(), 0, 128 * 4, s));
        gt_.cap = slots;
        gt_.rep = 1;
        build_rows_table_ = true;
    }
    PA_REQUIRE(build_rows_table_ && gt_.cap == slots && brow_occ_word_ == ki.occ_word, PA_ERR_DEVICE, "internal: build-row table mixed with another table");
    a.gt_tag = gt_.tag.as<uint64_t>();
    a.gt_keys = gt_.keys.as<uint64_t>();
    a.gt_words = gt_.words.as<uint64_t>();
    a.gt_mask = gt_.cap - 1;  // capacity - 1 (no mask: the slot is the build position)
    a.gt_max_fill = INT32_MAX;
    a.gt_rep_mask = 0;
    a.gt_rep_count = gt_.rep_count.as<int32_t>();
    const int64_t n = dp.n - start_row;
    if (n <= 0) return true;
    advance_columns(a, dp, start_row);
    a.n = n;
    // every wave walks one contiguous range of the page and all ranges are equally long: two rounds of as many workgroups as
    // the device holds at once (a grid that is not a multiple of that leaves CUs idle in the last round)
    int resident = 4;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&resident, ck.kernel.fn, ki.block, 0) != hipSuccess || resident <= 0) resident = 4;
    int per_cu = resident * 2;
    if (const char* e = getenv("PRESTO_AMD_BROW_GRID")) per_cu = std::max(1, atoi(e));  // (measurement switch: workgroups per CU)
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(((n + 3) / 4 + 255) / 256, (int64_t)cus_ * per_cu));
    void* params[] = {&a};
    timer.set_name(ck.kernel.name);
    timer.begin(s);
    PA_HIP(hipModuleLaunchKernel(ck.kernel.fn, grid, 1, 1, ki.block, 1, 1, 0, s, params, nullptr));
    timer.end(s);
    brow_keys_ = &ck;
    return true;
}

// the column pointers of `a` moved to row `offset` of the page
void FusedAggregationOperator::advance_columns(PaFusedArgs& a, const DevPage& dp, int64_t offset) const
{
    if (offset <= 0) return;
    for (int c = 0; c < spec_.n_in; c++) {
        if (!spec_.used_channel[c]) continue;
        const DevColumn& col = dp.cols[c];
        if (col.varwidth) a.o[c] = col.offsets + offset;
        else a.v[c] = static_cast<const char*>(col.values) + offset * type_width(col.type);
        if (col.nulls) a.nl[c] = col.nulls + offset;
    }
}

// One page -- or the rows of `list`, or the rows from start_row on -- through the kernel of one tier: fills what every tier's kernel
// is told about the page and hands over to the tier's launcher.
// returns false when the tier gave up and the rest of the page must be redone on the tier mode_ now names (see run_tiers)
bool FusedAggregationOperator::run_page(const Compiled& ck, const DevPage& dp, bool vec, const RowList* list, int64_t start_row)
{
    hipStream_t s = stream_.get();
    const KernelInfo& ki = ck.info;
    last_info_ = &ki;
    PaFusedArgs a;
    memset(&a, 0, sizeof a);
    for (int c = 0; c < spec_.n_in; c++) {
        if (!spec_.used_channel[c]) continue;
        a.v[c] = dp.cols[c].values;
        a.o[c] = dp.cols[c].offsets;
        a.nl[c] = dp.cols[c].nulls;
    }
    a.vec = vec ? 1 : 0;
    a.err = ctl_;
    a.gt_count = ctl_ + 1;
    a.overflow_rows = reinterpret_cast<uint64_t*>(ctl_ + 2);
    if (spec_.join) {
        fill_probe_args(a, *spec_.join);
        a.jrows = spec_.join->ls->n();
    }
    if (ki.variant == V_BROW) return run_page_build_rows(ck, dp, a, start_row);
    // a table of ranges: one launch takes all of them, a workgroup per entry at a time
    int64_t range_entries = 0;
    if (dp.ranges) {
        PA_REQUIRE(ki.ranged && !list && start_row == 0, PA_ERR_DEVICE, "internal: range table handed to a kernel that walks one page");
        range_entries = fill_range_table(ki, dp, a, s);
    }
    const int64_t offset = list ? list->first_row : start_row;
    const int64_t total = list ? list->first_row + list->chunk_rows : dp.n;
    if (ki.variant == V_GLOBAL) return launch_global(ck, dp, a, offset, total, range_entries);
    if (ki.variant == V_LDS) return launch_lds(ck, dp, a, vec, offset, total, range_entries);
    return launch_table(ck, dp, a, list, offset, total);
}

// Ungrouped tier (V_GLOBAL, its range-table and staged forms): one launch over rows [offset, total), one partial state per workgroup
// in the slab, merged into the state in a fixed order.
bool FusedAggregationOperator::launch_global(const Compiled& ck, const DevPage& dp, PaFusedArgs& a, int64_t offset, int64_t total, int64_t range_entries)
{
    if (offset >= total) return true;
    hipStream_t s = stream_.get();
    const KernelInfo& ki = ck.info;
    const int64_t n = total - offset;
    advance_columns(a, dp, offset);
    a.n = n;
    const int64_t work = dp.ranges ? range_entries * ki.block : (n + 3) / 4;  // (a workgroup per entry of a range table)
    const int grid = std::max((int)std::min<int64_t>((work + 255) / 256, (int64_t)cus_ * 8), 1);
    // (a staged kernel counts its rows alive behind the partial states: staged_decide)
    const size_t stage_words = ki.stage_bytes.empty() ? 0 : ki.stage_bytes.size() - 1;
    a.slab = static_cast<uint64_t*>(slab_.ensure((size_t)grid * (ki.nw + stage_words) * 8));
    if (!state_.ptr()) {
        state_.ensure((size_t)ki.nw * 8);
        PA_HIP(hipMemsetAsync(state_.ptr(), 0, (size_t)ki.nw * 8, s));
    }
    void* params[] = {&a};
    timer.set_name(ck.kernel.name);
    timer.begin(s);
    PA_HIP(hipModuleLaunchKernel(ck.kernel.fn, grid, 1, 1, ki.block, 1, 1, 0, s, params, nullptr));
    timer.end(s, true);
    // (on the main stream: moved to a second stream behind an event, as the few-groups tier's merges are, the 8 us kernel left the
    // gap between two launches what the timer's and the event's markers make it -- 39 instead of 43 us per Q6 pass)
    launch_merge_global_slab(a.slab, grid, ki.nw, ck.kinds.as<int32_t>(), state_.as<uint64_t>(), ctl_, s);
    if (!ki.stage_bytes.empty()) staged_decide(ck, a.slab, grid, a.vec ? (n & ~(int64_t)3) : 0, s);
    return true;
}

// Few-groups tier (V_LDS and its range-table form): per-wave partial tables in one of two slabs, merged into the HBM table on a
// second stream while the next launch streams; every launch is confirmed late (confirm_oldest).
bool FusedAggregationOperator::launch_lds(const Compiled& ck, const DevPage& dp, PaFusedArgs& a, bool vec, int64_t offset, int64_t total,
                                          int64_t range_entries)
{
    hipStream_t s = stream_.get();
    const KernelInfo& ki = ck.info;
    // head = leading multiple of 256 rows through the vector kernel, tail = the rest through the scalar one
    // (a range table has its tails inside: the one kernel takes everything)
    const int64_t lds_head = dp.ranges ? total : vec ? (total & ~(int64_t)255) : 0;
    while (offset < total) {
        int64_t n = total - offset;
        bool use_tail = false;
        if (offset < lds_head) {
            n = lds_head - offset;
            // nothing is known about the cardinality yet: a short first launch decides whether the register-table
            // variant fits, instead of a whole wasted pass over a large page
            if (!lds_.probed && ck.lds_verdict.load(std::memory_order_relaxed) == 1) lds_.probed = true;
            lds_.compiled = &ck;
            if (!lds_.probed && n > ((int64_t)1 << 22) && !dp.ranges) n = (int64_t)1 << 20;
        }
        else use_tail = true;
        advance_columns(a, dp, offset);
        a.n = n;
        int64_t work = use_tail ? n : (n + 3) / 4;
        if (dp.ranges) work = range_entries * ki.block;  // a workgroup per entry
        const int per_cu = std::max(1, std::min(16, (int)(160 * 1024 / ((size_t)ki.nw * ki.c * 64 * 8 + 512))));
        const int grid = std::max((int)std::min<int64_t>((work + 63) / 64, (int64_t)cus_ * per_cu), 1);
        const int b = lds_.page & 1;
        if (!lds_.merge_stream) {
            lds_.merge_stream = pool_stream_acquire();
            for (int i = 0; i < 2; i++) {
                PA_HIP(hipEventCreateWithFlags(&lds_.ev_main[i], hipEventDisableTiming));
                PA_HIP(hipEventCreateWithFlags(&lds_.ev_merge[i], hipEventDisableTiming));
            }
        }
        // slab b, its overflow word and lds_.ev_main[b] belong to launch k-2 until that one is confirmed
        while (lds_.inflight.size() >= kMaxInflight) confirm_oldest();
        if (mode_ != V_LDS) {  // a confirmation moved the operator to the next tier: the rows from here on go there
            resume_from_ = offset;
            return false;
        }
        // slab b was last read by the merge of page k-2
        if (lds_.merge_pending[b]) PA_HIP(hipStreamWaitEvent(s, lds_.ev_merge[b], 0));
        a.slab = static_cast<uint64_t*>(lds_.slab[b].ensure((size_t)grid * ki.c * (1 + ki.w + ki.nw) * 8));
        a.overflow_rows = reinterpret_cast<uint64_t*>(ctl_ + 2 + 2 * b);
        // the merges of this launch and of the one still in flight add at most 2 * grid * C groups
        ensure_table(gt_.groups_upper + 2 * (uint64_t)grid * ki.c);
        a.gt_tag = gt_.tag.as<uint64_t>();
        a.gt_keys = gt_.keys.as<uint64_t>();
        a.gt_words = gt_.words.as<uint64_t>();
        a.gt_mask = gt_.cap ? gt_.cap - 1 : 0;
        a.gt_max_fill = (int32_t)(gt_.cap - gt_.cap / 4);
        a.gt_rep_count = gt_.rep_count.as<int32_t>();
        void* params[] = {&a};
        if (!use_tail) timer.set_name(ck.kernel.name);
        timer.begin(s);
        PA_HIP(hipModuleLaunchKernel(use_tail ? ck.tail_kernel.fn : ck.kernel.fn, grid, 1, 1, ki.block, 1, 1, 0, s, params, nullptr));
        timer.end(s, !use_tail);
        // The merge skips itself when the launch overflowed (overflow_rows != 0).  It runs on the merge
        // stream, overlapped with the next page's fused kernel.  The control block (error word, group count, overflow
        // counters) is copied for the host behind the merge, on that stream too, when the launch is confirmed late anyway:
        // the main stream then carries nothing between two pages' fused kernels.  A launch the host waits for at once -- the
        // first of all, or one over a page that cannot be read again -- keeps its copy behind the kernel: the wait is for
        // the kernel alone.
        const bool late_ctl = lds_.probed && retained_;
        if (!late_ctl) PA_HIP(hipMemcpyAsync(h_ctl_lds(b), ctl_, 32, hipMemcpyDeviceToHost, s));
        PA_HIP(hipEventRecord(lds_.ev_main[b], s));
        PA_HIP(hipStreamWaitEvent(lds_.merge_stream, lds_.ev_main[b], 0));
        launch_merge_lds_slab(a.slab, grid, ki.c, ki.w, ki.nw, ck.kinds.as<int32_t>(), a.gt_tag, a.gt_keys, a.gt_words, a.gt_mask,
                              a.gt_max_fill, a.gt_count, ctl_, a.overflow_rows,
                              static_cast<int32_t*>(lds_.entry_slot[b].ensure((size_t)grid * ki.c * 4)), lds_.merge_stream);
        if (late_ctl) PA_HIP(hipMemcpyAsync(h_ctl_lds(b), ctl_, 32, hipMemcpyDeviceToHost, lds_.merge_stream));
        PA_HIP(hipEventRecord(lds_.ev_merge[b], lds_.merge_stream));
        lds_.merge_pending[b] = true;
        lds_.page++;
        // The launch is confirmed later: its overflow word says whether a wave met more groups than its register table
        // holds -- the merge then skipped itself and the rows are redone on the next tier.  The host only ever waits
        // for a launch when the page cannot be read again later (not retained), or for the first launch of all, whose
        // outcome decides the tier of everything that follows.
        Inflight f;
        f.b = b;
        f.dp = dp;
        f.dp.n = (int32_t)(offset + n);
        f.vec = vec;
        f.offset = offset;
        f.sig = *cur_sig_;
        f.layout = *cur_layout_;
        f.seq = ++lds_.launch_seq;
        f.late_ctl = late_ctl;
        lds_.inflight.push_back(std::move(f));
        if (!lds_.probed) {
            // the first launch of all: when it gives up, its rows are not redone on their own -- the page goes to the next
            // tier from this launch's first row on, so that the tier's own probe sees a whole page in front of it
            confirm_all_but_last();
            if (!confirm_oldest(false)) {
                resume_from_ = offset;
                return false;
            }
        }
        else if (!retained_) confirm_all();
        else poll_inflight();
        if (mode_ != V_LDS) {
            resume_from_ = offset + n;
            return false;
        }
        offset += n;
        if (resume_from_ >= 0) return false;  // the rest of the page goes to another tier (see run_tiers)
    }
    return true;
}

// workgroups of a launch of the table tiers over `work` work items
int FusedAggregationOperator::grid_for(const KernelInfo& ki, int64_t work, const RowList* list) const
{
    int grid;
    if (ki.variant == V_LDSP) {
        grid = ldsp_.parts;  // one workgroup per partition, whatever the page holds
    }
    else if (ki.variant == V_LDSH) {
        grid = (int)std::min<int64_t>((work + ki.block - 1) / ki.block, (int64_t)cus_ * (ki.block == 1024 ? 1 : 2));  // LDS per CU: 160 KB
        // partition-ordered rows: at least one workgroup per partition, so that a workgroup's table meets the groups of
        // one partition (not of the two or three its slice would span with a workgroup per CU)
        if (list && ldsp_.list_grid_hint > grid) grid = (int)std::min<int64_t>((work + ki.block - 1) / ki.block, (int64_t)ldsp_.list_grid_hint);
    }
    else {
        grid = (int)std::min<int64_t>((work + 255) / 256, (int64_t)cus_ * 8);
    }
    return std::max(grid, 1);
}

// replicas of the HBM table for a launch of `grid` workgroups
uint32_t FusedAggregationOperator::replicas_for(const KernelInfo& ki, int grid, const RowList* list) const
{
    if (ki.variant == V_LDSP) return gt_.rep;  // the HBM table only takes the rows that fall through
    uint32_t want = desired_replicas(gt_.probed ? gt_.groups_upper : std::max<uint64_t>(gt_.groups_upper, (uint64_t)std::max(spec_.expected_groups, 1)));
    // (the LDS-table tier reaches the HBM table once per group and workgroup, its workgroups each starting elsewhere in
    // their tables: a few replicas are plenty, and every replica is memory to clear and a table to fold at the end)
    if (ki.variant == V_LDSH) want = std::min<uint32_t>(want, kLdshReplicas);
    // change the layout only when it pays: much more replication needed, or far too much held
    uint32_t reps = (want >= 2 * gt_.rep || want * 4 <= gt_.rep) ? want : gt_.rep;
    reps = std::min<uint32_t>(reps, next_pow2((uint64_t)grid));
    // the launch that tells the cardinality counts into ONE table: the groups of replicas cannot be told apart from
    // the outside (their sum counts a group once per replica that met it), and its few workgroups' flushes are
    // no load on anybody's addresses
    if (ki.variant == V_LDSH && !gt_.probed && !list && gt_.groups_upper == 0) reps = 1;
    return reps;
}

// the arguments of the launch that replays the `spilled` rows listed in spill[cur], on the table as ensure_table has just left it
PaFusedArgs FusedAggregationOperator::replay_args(const PaFusedArgs& a, uint32_t spilled, int cur, uint64_t flush_room)
{
    PaFusedArgs r = a;
    r.n = 0;
    if (r.list_blocked == 2) r.list_blocked = 1;  // the spilled rows are a real list
    r.row_list = gt_.spill[cur].as<int32_t>();
    r.n_list = spilled;
    r.spill_rows = static_cast<int32_t*>(gt_.spill[cur ^ 1].ensure((size_t)spilled * 4));
    r.gt_tag = gt_.tag.as<uint64_t>();
    r.gt_keys = gt_.keys.as<uint64_t>();
    r.gt_words = gt_.words.as<uint64_t>();
    r.gt_mask = gt_.cap - 1;
    r.gt_max_fill = (int32_t)(gt_.cap / 2 - flush_room);
    return r;
}

// Table tiers (V_GT: the HBM table itself; V_LDSH / V_LDSP: workgroup-level LDS tables in front of it): launches of at most 2^26
// rows, each followed by the replay of the rows whose group found no room, and by the decision which tier takes the rows behind it.
bool FusedAggregationOperator::launch_table(const Compiled& ck, const DevPage& dp, PaFusedArgs& a, const RowList* list, int64_t offset, int64_t total)
{
    hipStream_t s = stream_.get();
    const KernelInfo& ki = ck.info;
    // the HBM-table variant bounds the groups one launch can add so that the table can be sized first
    const int64_t chunk = (int64_t)1 << 26;
    while (offset < total) {
        int64_t n = std::min(chunk, total - offset);
        // the first launch on the HBM table is a short one: it tells how many groups there are, which decides the
        // number of table replicas for the rest
        // (the distinct keys of 2^18 rows tell hundreds of groups from hundreds of thousands, and -- by how many of the rows
        // were new keys, estimate_groups -- those from millions; the rows of a probe that sends the page to the
        // partition-owned tables are redone there -- see lone_probe)
        if (!gt_.probed && !list) n = std::min<int64_t>(n, kProbeRows);
        advance_columns(a, dp, offset);
        a.n = list ? 0 : n;
        int64_t work = (n + 3) / 4;
        if (list) {
            a.row_list = list->rows;
            a.n_list = list->count;
            a.list_blocked = list->rows ? 1 : 2;  // 2: rows 0 .. count-1 of (reordered) columns, one contiguous slice per workgroup
            work = list->count;
        }
        const int grid = grid_for(ki, work, list);
        const uint32_t reps = replicas_for(ki, grid, list);
        // V_LDSH: every workgroup adds up to lc / 2 groups of its LDS table at the end of the launch, and must find room
        auto room_for_flush = [&](uint32_t r) { return ki.variant == V_LDSH ? (uint64_t)((grid + r - 1) / r) * (uint64_t)(ki.lc / 2) : (uint64_t)0; };
        uint64_t flush_room = room_for_flush(reps);
        drain_merges();
        // sized by the groups seen so far, not by the rows: rows whose new group does not fit are spilled and
        // replayed after a rehash (see below)
        // (ensure_table doubles its argument: the table is kept at most half full)
        // (partition-owned tables: the HBM table only takes what falls through -- no need to size it for the estimate)
        const uint64_t expected = ki.variant == V_LDSP ? 0 : (uint64_t)std::max(spec_.expected_groups, 0);
        ensure_table(std::max<uint64_t>({(uint64_t)16384 / reps, gt_.groups_upper + gt_.groups_upper / 4, expected}) + flush_room, reps);
        if (gt_.rep != reps) {  // the memory bound reduced the replicas
            flush_room = room_for_flush(gt_.rep);
            ensure_table(std::max<uint64_t>({(uint64_t)16384 / gt_.rep, gt_.groups_upper + gt_.groups_upper / 4, expected}) + flush_room);
        }
        a.spill_rows = static_cast<int32_t*>(gt_.spill[0].ensure((size_t)n * 4));
        a.spill_count = reinterpret_cast<uint32_t*>(ctl_ + 6);
        if (!list) {
            a.row_list = nullptr;
            a.n_list = 0;
        }
        a.gt_tag = gt_.tag.as<uint64_t>();
        a.gt_keys = gt_.keys.as<uint64_t>();
        a.gt_words = gt_.words.as<uint64_t>();
        a.gt_mask = gt_.cap ? gt_.cap - 1 : 0;
        a.gt_max_fill = (int32_t)(gt_.cap / 2 - flush_room);
        a.gt_rep_mask = gt_.rep - 1;
        if (ki.variant == V_LDSP) {
            a.sub_tag = ldsp_.tag.as<uint64_t>();
            a.sub_keys = ldsp_.keys.as<uint64_t>();
            a.sub_words = ldsp_.words.as<uint64_t>();
            a.sub_count = ldsp_.count.as<int32_t>();
            a.part_first = ldsp_.part_first.as<int64_t>();
            a.row_list = nullptr;
            a.n_list = 0;
            a.list_blocked = 0;
            a.pad3 = ldsp_.fresh ? 1 : 0;
            ldsp_.fresh = false;
        }
        a.gt_rep_count = gt_.rep_count.as<int32_t>();
        void* params[] = {&a};
        timer.set_name(ck.kernel.name);
        timer.begin(s);
        PA_HIP(hipModuleLaunchKernel(ck.kernel.fn, grid, 1, 1, ki.block, 1, 1, 0, s, params, nullptr));
        timer.end(s, true);
        // replay loop: grow the table until every row of the launch found room for its group
        int cur = 0;
        // the launch that tells the cardinality, on a table that held nothing before it
        const bool lone_probe = !gt_.probed && !list && gt_.groups_upper == 0 && gt_.groups_sum == 0 && ldsp_.parts == 0 && !is_combiner_;
        for (;;) {
            read_group_counts(s);
            raise_if(h_ctl_[0]);
            const bool first_probe = !gt_.probed;
            gt_.probed = true;
            const uint32_t spilled = (uint32_t)h_ctl_[6];
            if (ki.variant == V_LDSP) {
                uint64_t fell;
                memcpy(&fell, h_ctl_ + 2, 8);
                if (fell != 0) PA_HIP(hipMemsetAsync(ctl_ + 2, 0, 8, s));
                ldsp_.fell += fell;
            }
            if (ki.variant == V_LDSH) {
                // rows that found no room in the workgroups' LDS tables: when they are a large part of the
                // page, the cardinality is beyond this variant and later pages go to the HBM table directly
                uint64_t fell;
                memcpy(&fell, h_ctl_ + 2, 8);
                if (fell != 0) PA_HIP(hipMemsetAsync(ctl_ + 2, 0, 8, s));
                if (fell > (uint64_t)n / 4) mode_ = V_GT;
                // the probe launch is short -- its workgroups' tables have room for all they see -- so the groups it
                // found speak instead: more than a workgroup's table takes, and the tiers behind the HBM table's probe
                // (hash-partitioned LDS tables, partition-owned tables) do better from the next row on
                if (lone_probe && first_probe && estimate_groups(gt_.groups_sum, (uint64_t)n) > (uint64_t)ki.lc / 2) mode_ = V_GT;
            }
            if (spilled == 0) {
                // (also after replays of spilled rows: the rest of the page must not crawl through the wrong tier)
                if (ki.variant == V_LDSH && mode_ == V_GT && !list && offset + n < total) resume_from_ = offset + n;
                // the probe launch on the HBM table has told the cardinality: when it calls for the hash-partitioned
                // tiers, the rest of this page already goes there
                if (ki.variant == V_GT && first_probe && !list && offset + n < total && mode_ == V_GT) {
                    int p = 0;
                    if (partitioned_wanted(*cur_sig_, *cur_layout_, &p)) resume_from_ = offset + n;
                }
                // ... and when it calls for the partition-owned tables, the probe's own groups are given up: left in the
                // HBM table they would make every group of the partitions' tables pay an upsert there at the end (the
                // fold: 0.24 ms for 1 M groups), where redoing the probe's rows with the rest of the page costs a few
                // per cent of the page
                if (lone_probe && resume_from_ >= 0 && mode_ == V_GT && !getenv("PRESTO_AMD_KEEP_PROBE")) {
                    int p = 0;
                    gt_.probed_groups = std::max(gt_.probed_groups, estimate_groups(gt_.groups_sum, (uint64_t)n));
                    if (partitioned_wanted(*cur_sig_, *cur_layout_, &p) && ldsp_.want) {
                        drop_table();
                        resume_from_ = offset;
                    }
                }
                break;
            }
            PA_HIP(hipMemsetAsync(ctl_ + 6, 0, 4, s));
            // at least twice the slots (ensure_table doubles its argument)
            ensure_table(std::max<uint64_t>((uint64_t)gt_.cap / 2 + 1, gt_.groups_upper + spilled) + flush_room);
            PaFusedArgs r = replay_args(a, spilled, cur, flush_room);
            void* rparams[] = {&r};
            // (never more workgroups than the launch the table was sized for: V_LDSH flushes per workgroup)
            // partition-owned tables: the spilled rows are a list over all partitions -- they go to the HBM table, through its kernel
            const Compiled& rk = ki.variant == V_LDSP ? kernel_for(*cur_sig_, *cur_layout_, V_GT) : ck;
            int rgrid = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)spilled + rk.info.block - 1) / rk.info.block, (int64_t)grid));
            timer.begin(s);
            PA_HIP(hipModuleLaunchKernel(rk.kernel.fn, rgrid, 1, 1, rk.info.block, 1, 1, 0, s, rparams, nullptr));
            timer.end(s);
            cur ^= 1;
        }
        offset += n;
        if (resume_from_ >= 0) return false;  // the rest of the page goes to another tier (see run_tiers)
    }
    return true;
}


// confirms the launches whose kernel has finished, without waiting
void FusedAggregationOperator::poll_inflight()
{
    while (!lds_.inflight.empty()) {
        const Inflight& f = lds_.inflight.front();
        if (hipEventQuery(f.late_ctl ? lds_.ev_merge[f.b] : lds_.ev_main[f.b]) != hipSuccess) break;
        confirm_oldest();
    }
    (void)hipGetLastError();  // hipErrorNotReady is not an error here
}

void FusedAggregationOperator::confirm_all()
{
    while (!lds_.inflight.empty()) confirm_oldest();
}

void FusedAggregationOperator::confirm_all_but_last()
{
    while (lds_.inflight.size() > 1) confirm_oldest();
}

// false: the launch met more groups than its tier takes (redo: its rows are redone on the next tier here and now)
bool FusedAggregationOperator::confirm_oldest(bool redo)
{
    Inflight f = std::move(lds_.inflight.front());
    lds_.inflight.pop_front();
    // The launch's control block as it was behind its kernel (ev_main) or, late_ctl, behind its merge (ev_merge).  Either copy
    // tells the same about the launch: its overflow word is written by the fused kernel alone -- the merge only reads it, to skip
    // itself -- and a later launch has a word of its own until this one is confirmed.  The group count differs: behind the merge it
    // includes this launch's groups, so groups_upper is exact for every confirmed launch and only the unconfirmed ones (at most
    // kMaxInflight, counting the launch about to be made) add their grid * C each -- what launch_lds sizes the table for.
    PA_HIP(hipEventSynchronize(f.late_ctl ? lds_.ev_merge[f.b] : lds_.ev_main[f.b]));
    const int32_t* hc = h_ctl_lds(f.b);
    uint64_t overflow;
    memcpy(&overflow, hc + 2 + 2 * f.b, 8);
    raise_if(hc[0]);
    if (overflow == 0) {
        gt_.groups_upper = std::max<uint64_t>(gt_.groups_upper, (uint64_t)hc[1]);  // groups merged so far (in-flight merges are bounded above)
        lds_.probed = true;
        if (lds_.compiled) lds_.compiled->lds_verdict.store(1, std::memory_order_relaxed);
        return true;
    }
    if (lds_.compiled) lds_.compiled->lds_verdict.store(2, std::memory_order_relaxed);
    // more groups than the wave's register table: the launch's merge skipped itself; its rows -- and every later page --
    // go to the workgroup-level LDS table, which itself hands rows it has no room for to the HBM table
    hipStream_t s = stream_.get();
    last_valid_ = false;  // (the redo goes to the stream behind whatever finish() recorded)
    drain_merges();
    PA_HIP(hipMemsetAsync(ctl_ + 2 + 2 * f.b, 0, 8, s));
    if (mode_ == V_LDS) mode_ = V_LDSH;
    if (!redo) return false;
    const int64_t saved = resume_from_;
    const bool saved_retained = retained_;
    retained_ = false;
    run_tiers(f.sig, f.layout, f.dp, f.vec, f.offset);
    retained_ = saved_retained;
    resume_from_ = saved;
    return false;
}

}  // namespace fused_op
}  // namespace pa
