// op_fused.hpp -- the fused scan-filter-project-aggregate operator's class (host side): its nested types, its data members grouped by
// the concern that owns them, and its member functions' declarations.  Only bodies of a line or two that run per page or per poll are
// defined here.  See op_fused.cpp for what the operator replaces, the kernel tiers and which of the op_fused_*.cpp files defines what.
// Included by those files only.
#pragma once

#include <atomic>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "exchange_kernels.hpp"
#include "fused_plan.hpp"
#include "intern_kernels.hpp"
#include "jit.hpp"
#include "join_source.hpp"
#include "operator.hpp"
#include "scan_kernels.hpp"
#include "static_kernels.hpp"

namespace pa {

using namespace fused;

namespace fused_op {

inline uint32_t next_pow2(uint64_t v)
{
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return (uint32_t)p;
}

class FusedAggregationOperator : public pa_operator {
public:
    explicit FusedAggregationOperator(const pa_fused_aggregation_desc* d);
    FusedAggregationOperator(Spec spec, void* stream);
    ~FusedAggregationOperator() override;
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }

    // ---- Operator protocol with device work in flight (op_fused.cpp) -----------------------------------------------------
    // add_input only enqueues.  Small pages are gathered first (see "small pages" below); the fused launches of the few-groups
    // variant are confirmed one launch late (its overflow word decides whether a launch must be redone on the next tier), so
    // the host is one launch ahead of the device and never waits inside add_input for a stable page.  needs_input() turns
    // false -- and is_blocked() true -- while two launches are unconfirmed (Operator.isBlocked, Operator.java:69-80): the
    // Driver polls, as it does for a future, instead of parking a thread in the native call.
    // probe stage: no page is taken before the build side has published its lookup source (LookupJoinOperator.needsInput /
    // isBlocked on the lookup source future, LookupJoinOperator.java:63, 100)
    bool takes_retained() override { return true; }
    bool needs_input() override
    {
        poll_releases();
        if (finishing_) return false;
        if (!lookup_source_ready()) return false;
        if (!retry_parked()) return false;
        if (next_) return next_->needs_input();
        poll_inflight();
        return lds_.inflight.size() < kMaxInflight;
    }
    bool is_blocked() override
    {
        if (!lookup_source_ready()) return !finishing_;
        if (!retry_parked()) return true;  // waiting for HBM (Operator.isBlocked on a memory future, Operator.java:69-80)
        if (next_) return next_->is_blocked();
        poll_inflight();
        return lds_.inflight.size() >= kMaxInflight;
    }
    void add_input(const pa_page* page) override;
    void finish() override;
    bool is_finished() override { return finishing_ && output_done_; }
    bool get_output(pa_page* out) override;
    // The consumer of this operator's output is a TopN(n; sort channels / orders over the OUTPUT channels): groups that cannot be
    // among its n best rows may be left out (pa_aggregation_set_output_topn_hint).
    bool set_output_topn(int64_t n, const int32_t* channels, const int32_t* orders, int32_t count) override;
    int64_t memory_bytes() override
    {
        return (int64_t)(stager_.bytes() + slab_.capacity() + gt_.tag.capacity() + gt_.keys.capacity() + gt_.words.capacity() + state_.capacity());
    }
    // What isFull() compares with maxPartialMemory: the groups known so far x the bytes of a group's key and state words (and
    // its table slot), over all generations.  Launches still unconfirmed are not counted yet.
    int64_t group_bytes();
    const Spec& spec() const { return spec_; }
    void* stream_handle() { return stream_.get(); }

private:
    // ==== nested types ====================================================================================================
    struct TopNHint {
        int64_t n = 0;
        std::vector<int32_t> channels, orders;
    };
    // PA_PAGE_RETAINED: the page's owner keeps its buffers valid and unchanged until this operator calls page->release(ctx) -- what a
    // reference does for a Java Page.  Such a page is taken like a stable one (merged into a range, listed in a range table, copied
    // into the arena at the arena's launch -- no launch and no wait per page); its release travels with the structure the page went
    // to and is called, from inside a later call on this handle, once the launches that read the page have finished AND been
    // confirmed (a few-groups launch that met too many groups is redone from the same buffers, confirm_oldest).
    struct Release {
        void (*fn)(void*) = nullptr;
        void* ctx = nullptr;
    };
    struct ReleaseBatch {
        hipEvent_t event = nullptr;
        uint64_t seq = 0;            // 0: the event alone decides; else every few-groups launch up to this one must be confirmed
        std::vector<Release> rel;
    };
    // One code object + word-kind table per (plan fingerprint, column-layout signature, variant, device), shared by every
    // operator instance of the process: an operator lives for one query (OperatorFactory.createOperator), the generated
    // code for its plan node does not change -- re-generating ~30 KB of source and hashing it per instance cost ~0.1 ms.
    struct Compiled {
        KernelInfo info;
        JitKernel kernel, tail_kernel;
        DevBuf kinds;
        // V_LDS: what the first launch of earlier operators of this plan found -- 1: every wave's register table held its groups,
        // 2: one overflowed.  An operator that finds 1 here does not cut a short probe launch off its first page and wait for it:
        // the whole page goes out and is confirmed late, like every later page (a wrong guess is the redo path of confirm_oldest).
        mutable std::atomic<int> lds_verdict{0};
        // V_GLOBAL_S: what the first launch of this plan's staged kernel predicted -- 1: the staged loads move at most kStagedGain
        // of the bytes the plain loop moves, the staged kernel stays; 2: they do not, the plain kernel takes over
        mutable std::atomic<int> staged_verdict{0};
    };
    // rows of one chunk of a page in a given order (the hash-partitioned path)
    struct RowList {
        const int32_t* rows;   // positions relative to the chunk's first row
        int64_t count;
        int64_t first_row;     // of the chunk in the page
        int64_t chunk_rows;
    };
    // a few-groups launch not confirmed yet
    struct Inflight {
        int b = 0;            // slab / overflow word / event pair of the launch
        DevPage dp;           // the page, cut at the end of the launched rows
        bool vec = false;
        int64_t offset = 0;   // first row of the launch
        std::string sig;
        std::vector<ChannelLayout> layout;
        uint64_t seq = 0;     // position among the operator's few-groups launches (release_checkpoint)
        bool late_ctl = false;  // its control block is copied behind its merge, on the merge stream: lds_.ev_merge[b] confirms it
    };
    // the pending range of stable device pages that continue each other in memory
    struct Run {
        int64_t rows = 0;
        bool flat = true;                 // every used channel is FLAT (a small range can join the arena)
        std::vector<pa_column> cols;      // first page of the range: every later page continues these buffers
    };
    struct RangeTable {
        PinnedBuf host;
        DevBuf dev;
        hipEvent_t event = nullptr;
        bool used = false;
    };
    struct Arena {
        int64_t rows = 0;
        std::vector<bool> nullable;
        std::vector<DevBuf> values, nulls, offsets;   // per channel; VARCHAR: values = bytes, offsets = rows + 1 entries
        std::vector<int64_t> bytes;                   // VARCHAR bytes used
        std::vector<CopySeg> segs;                    // copies of stable, device-readable pages, done at the arena's launch
        std::vector<Release> rel;                     // releases of the retained pages copied (or to be copied) into this arena
        PinnedBuf h_table;
        DevBuf d_table;
        hipEvent_t table_event = nullptr;
        bool table_used = false;
        // VariableWidthBlocks of device pages (launch_var_append): the byte cursors live in HBM, two halves used in turn
        bool dev_var = false, var_fresh = true;
        int cursor_half = 0;
        DevBuf cursors;
        std::vector<VarSeg> vsegs;                    // deferred appends (stable pages), done at the arena's launch
        PinnedBuf h_vtable;
        DevBuf d_vtable;
        hipEvent_t vtable_event = nullptr;
        bool vtable_used = false;
    };
    // per ranked channel (Spec::ranked): the dictionary's strings on the host, their ids in string order, the ranks on the device, the
    // page's image column
    struct RankedChannel {
        std::vector<std::string> strings;
        std::vector<uint32_t> order;
        DevBuf ranks, image;
    };

    // ==== Operator protocol, parked pages, generations (op_fused.cpp) ====================================================
    bool lookup_source_ready() const { return !spec_.join || spec_.join->ls->built.load(); }
    // A page whose buffers stay valid after add_input returns: PA_PAGE_STABLE (until the operator is closed) or PA_PAGE_RETAINED
    // (until the operator calls the page's release -- see "retained pages" below)
    static bool page_stays(const pa_page* page) { return (page->flags & (PA_PAGE_STABLE | PA_PAGE_RETAINED)) != 0; }
    bool retry_parked();
    void take_page(const pa_page* page);
    void process_page(const pa_page* page, bool retained);
    void start_next_generation();
    bool emit_states(pa_page* out);
    bool combine_generations(pa_page* out);
    Spec combiner_spec() const;
    static void raise_if(int32_t code);  // the device's error word as an Error

    // ==== retained pages, small pages, range tables (op_fused_pages.cpp) =================================================
    Release take_cur_release()
    {
        cur_rel_set_ = false;
        return cur_rel_;
    }
    void release_checkpoint(std::vector<Release> rel, bool needs_confirm);
    void poll_releases();
    void release_everything();
    // ---- small pages ----
    // An unmodified Driver hands over pages of <= 1 MB / 8192 rows (PageProcessor.java:56-58); one launch per such page
    // would leave the device idle between launches.  Two ways out, both keeping add_input a plain enqueue:
    //  * consecutive STABLE device pages that continue each other in memory (row ranges of resident columns: Page.getRegion
    //    views, pages over one pinned / HBM staging area) are merged into one range -- no copy, only pointer compares -- and
    //    launched once the range holds kGatherRows rows (or at finish);
    //  * other small pages with fixed-width used channels are copied behind each other into one of two arenas (one H2D copy
    //    per column for host pages; one segment-copy launch per page for device pages, whose buffers may be recycled by their
    //    producer after add_input returns) and the arena is launched when it is full.
    static constexpr int64_t kSmallPageRows = (int64_t)1 << 21;
    // stable ranges below this many rows wait for each other in a range table (one launch for all of them); a range of 2^24 rows
    // -- 0.5 GB of Q6 columns -- pays for a launch and its merges of its own.  (Measured, profiles/r04_page_sweep.md: with the limit at
    // 2^21 rows, pages of 2^22 rows that do not continue each other got a launch each and ran at half the rate of 2^20-row pages.)
    static constexpr int64_t kRangeTableRows = (int64_t)1 << 24;
    static constexpr int64_t kArenaRows = (int64_t)1 << 22;
    static constexpr int64_t kDeviceVarMaxLength = 16;  // (see device_var_gatherable)
    static constexpr size_t kMaxRanges = 16384;
    static constexpr size_t kArenaMaxSegs = 16384;
    static int64_t gather_rows();
    bool channel_plain(const pa_column& col, int c) const
    {
        if (col.encoding == PA_FLAT) return col.type == spec_.in_types[c] || spec_.derived(c);
        return col.encoding == PA_VARWIDTH;
    }
    bool gather_small_page(const pa_page* page);
    bool device_var_gatherable() const;
    void retire_run();
    void flush_run();
    void append_to_arena(const pa_page* page);
    void flush_var_segments(Arena& a);
    void flush_arena();
    void flush_pending();
    // ---- range tables ----
    bool ranges_possible() const;
    void flush_ranges();
    void process_ranges(const std::shared_ptr<const std::vector<DevPage>>& set, int64_t rows);
    static bool range_aligned(const DevPage& r, const std::vector<bool>& used);
    int64_t fill_range_table(const KernelInfo& ki, const DevPage& dp, PaFusedArgs& a, hipStream_t s);

    // ==== launches: kernel cache, staged loads, the tiers (op_fused_launch.cpp) ==========================================
    void add_page(const pa_page* page);
    void run_tiers(const std::string& sig, const std::vector<ChannelLayout>& layout, const DevPage& dp, bool vec, int64_t start_row);
    static std::shared_ptr<const Compiled> shared_lookup(const std::string& key);
    static std::mutex& shared_mutex();
    static std::map<std::string, std::shared_ptr<const Compiled>>& shared_cache();
    const Compiled& kernel_for(const std::string& sig, const std::vector<ChannelLayout>& layout, int variant);
    void adopt_layout(const Compiled& c);
    // ---- staged loads (V_GLOBAL_S) ----
    // PRESTO_AMD_STAGED=0 | 1 | auto (default): never / always (whenever the plan stages its loads) / as the first launch predicts.
    // Under auto, launches of fewer than kStagedMinRows rows keep the plain kernel: the staged one is not worth a compilation there.
    static constexpr int64_t kStagedMinRows = (int64_t)1 << 22;
    static constexpr double kStagedGain = 0.85;
    static int staged_mode();
    const Compiled* staged_kernel(const std::string& sig, const std::vector<ChannelLayout>& layout, int64_t rows);
    static double staged_bytes(const std::vector<int>& w, const std::vector<double>& alive);
    void staged_decide(const Compiled& ck, const uint64_t* slab, int grid, int64_t vec_rows, hipStream_t s);
    // ---- one page through one tier: run_page fills the arguments every tier shares and hands over to the tier's launcher ----
    // (false: the tier gave up -- resume_from_ says from which row the tier mode_ now names takes over, see run_tiers)
    bool run_page(const Compiled& ck, const DevPage& dp, bool vec, const RowList* list = nullptr, int64_t start_row = 0);
    void advance_columns(PaFusedArgs& a, const DevPage& dp, int64_t offset) const;
    bool run_page_build_rows(const Compiled& ck, const DevPage& dp, PaFusedArgs a, int64_t start_row);
    bool launch_global(const Compiled& ck, const DevPage& dp, PaFusedArgs& a, int64_t offset, int64_t total, int64_t range_entries);
    bool launch_lds(const Compiled& ck, const DevPage& dp, PaFusedArgs& a, bool vec, int64_t offset, int64_t total, int64_t range_entries);
    bool launch_table(const Compiled& ck, const DevPage& dp, PaFusedArgs& a, const RowList* list, int64_t offset, int64_t total);
    int grid_for(const KernelInfo& ki, int64_t work, const RowList* list) const;
    uint32_t replicas_for(const KernelInfo& ki, int grid, const RowList* list) const;
    PaFusedArgs replay_args(const PaFusedArgs& a, uint32_t spilled, int cur, uint64_t flush_room);
    // ---- late confirmation of the few-groups launches ----
    static constexpr size_t kMaxInflight = 2;
    int32_t* h_ctl_lds(int b) const { return h_ctl_ + 16 + 8 * b; }
    void poll_inflight();
    void confirm_all();
    void confirm_all_but_last();
    bool confirm_oldest(bool redo = true);

    // ==== the HBM table and the hash-partitioned path on it (op_fused_table.cpp) =========================================
    static constexpr int64_t kProbeRows = (int64_t)1 << 18;  // the launch that tells the cardinality (see estimate_groups)
    static constexpr uint32_t kLdshReplicas = 4;
    static uint32_t desired_replicas(uint64_t g);
    void ensure_table(uint64_t min_groups, uint32_t reps = 0);
    static uint64_t estimate_groups(uint64_t d, uint64_t n);
    void drop_table();
    void read_group_counts(hipStream_t s);
    void drain_merges();
    bool partitioned_wanted(const std::string& sig, const std::vector<ChannelLayout>& layout, int* partitions);
    void run_page_partitioned(const std::string& sig, const std::vector<ChannelLayout>& layout, const DevPage& dp, bool vec, int partitions,
                              int64_t start_row);
    // where the group table keeps its tags / accumulator words (static_kernels.hpp, GtStrides)
    const uint64_t* table_tags() const
    {
        return build_rows_table_ && brow_occ_word_ >= 0 ? gt_.words.as<uint64_t>() + (size_t)brow_occ_word_ * gt_.cap : gt_.tag.as<uint64_t>();
    }
    const uint64_t* table_words() const { return gt_.words.as<uint64_t>(); }
    GtStrides table_strides() const { return GtStrides{1u, gt_.cap, 1u, 0u, build_rows_table_ && brow_occ_word_ >= 0 ? brow_occ_empty_ : 0ULL}; }

    // ==== VARCHAR keys as dictionary ids, ranks for min / max (op_fused_intern.cpp) ======================================
    void intern_keys(DevPage& dp, hipStream_t s);
    void intern_dictionary_key(const pa_page* page, int c, DevPage& dp, hipStream_t s);
    void decode_interned_keys();
    int interned_channel(int gi) const;
    void rank_values(DevPage& dp, hipStream_t s);
    void rerank_words(int c, const uint32_t* ranks, hipStream_t s);
    int ranked_channel(int proj) const;

    // ==== the result page (op_fused_output.cpp) ==========================================================================
    void build_output(bool eager = false);
    bool fetch_result(const KernelInfo& ki, std::vector<uint64_t>& keys, std::vector<uint64_t>& words, int64_t& groups);
    void assemble_output(const KernelInfo& ki, const std::vector<uint64_t>& keys, const std::vector<uint64_t>& words, int64_t groups);
    bool emit_on_device(const KernelInfo& ki, int64_t groups, bool keys_from_build_columns = false);
    // ---- the eager result: finish() enqueues, behind the operator's last launch, everything get_output needs of a small result -- the
    // control block, the ungrouped state or the compacted rows of at most kEagerGroups groups -- into pinned memory and records
    // eager_.event.  get_output waits for that event alone (never for the stream, which other operators share), validates what
    // landed (eager_result_holds) and assembles the page from it; a result that does not hold is dropped and fetch_result runs.
    // PRESTO_AMD_EAGER_OUTPUT=0 (read when the operator is made): nothing is enqueued at finish.
    // kEagerGroups stays below emit_on_device's threshold: a result is either eager or emitted on the device, never a choice.
    static constexpr int64_t kEagerGroups = 1024;
    static constexpr uint32_t kEagerTableSlots = 1u << 20;  // a larger table's scan is not spent on a guess
    bool eager_possible() const;
    void enqueue_eager_result();
    bool eager_result_holds();
    void take_eager_result(std::vector<uint64_t>& keys, std::vector<uint64_t>& words, int64_t& groups) const;
    // ---- the operator's own last work on the main stream: what the destructor waits for instead of the whole (shared) stream ----
    void mark_last_event();

    // ==== data members, by owner ==========================================================================================
    // Pooled buffers return to their caches in the members' destructors, after ~FusedAggregationOperator has drained the streams;
    // stream_ is declared in front of every buffer and so outlives them all.

    // ---- shared: read by every concern ----
    Spec spec_;
    Stream stream_;
    std::string plan_fingerprint_;
    bool grouped_ = false, finishing_ = false, output_done_ = false;
    int cus_ = 256;
    // the tier in charge.  Written by the constructor, add_page (V_BROW), run_tiers and the hand-over decisions of launch_table and
    // confirm_oldest; everybody else only reads it
    int mode_ = V_GLOBAL;
    DevBuf ctl_buf_;
    PinnedBuf h_ctl_buf_;
    int32_t* ctl_ = nullptr;    // device control block: [0] err  [1] gt_count  [2..5] overflow rows  [6] spill count
    int32_t* h_ctl_ = nullptr;  // its host copy [0..15], and one copy per slab of the LDS variant [16..31]

    // ---- Operator protocol, parked page, generations (op_fused.cpp) ----
    TopNHint topn_hint_;                  // (read by op_fused_output.cpp)
    bool out_partial_ = false;            // the output is the accumulator states (Step.PARTIAL, or a generation to be combined)
    std::vector<bool> nullable_seen_;     // per channel: some page so far carried a valueIsNull array (written by add_page / process_ranges)
    int generation_ = 0;
    bool is_combiner_ = false;
    std::unique_ptr<FusedAggregationOperator> next_;      // later generation: every page from the layout change on
    std::unique_ptr<FusedAggregationOperator> combiner_;  // FINAL-input operator over the generations' states
    bool parked_ = false;                 // a stable page waits for HBM (see retry_parked)
    pa_page parked_page_{};
    std::vector<pa_column> parked_cols_;
    size_t parked_need_ = 0;

    // ---- pages in: retained pages, small pages, range tables (op_fused_pages.cpp) ----
    PageStager stager_;                   // (add_page stages through it)
    PinnedPageCopy pinned_copy_;
    std::vector<int64_t> var_bytes_hint_; // per channel, while an arena of host pages is processed: bytes of its VARCHAR block (read by intern_keys)
    Release cur_rel_;                     // release of the page take_page is working on, until a structure takes it over
    bool cur_rel_set_ = false;
    std::vector<Release> run_rel_, ranges_rel_, carry_rel_;
    std::deque<ReleaseBatch> release_batches_;
    std::vector<hipEvent_t> release_events_;
    Run run_;
    std::shared_ptr<std::vector<DevPage>> ranges_;  // stable device ranges waiting to be launched as one table (see retire_run)
    int64_t range_rows_ = 0;
    RangeTable range_table_[3];
    int range_table_next_ = 0;
    Arena arena_[2];
    int arena_cur_ = 0;

    // ---- kernel cache, state layout, the page in run_page's hands (op_fused_launch.cpp) ----
    std::map<std::string, std::shared_ptr<const Compiled>> compiled_;
    bool layout_fixed_ = false;
    int nw_ = 0, w_ = 0;                  // accumulator / key words of a group (fixed by the first kernel, adopt_layout; read everywhere)
    std::string layout_id_;
    const int32_t* kinds_dev_ = nullptr;
    const KernelInfo* last_info_ = nullptr;  // layout of the accumulator words in the table (the last launch's; read by build_output)
    bool staged_refused_ = false;         // the plan stages its loads, but no staged kernel loads its columns
    bool join_checked_ = false;           // probe stage: the lookup source was looked at (first page)
    const std::string* cur_sig_ = nullptr;                  // signature / layout of the page run_page works on
    const std::vector<ChannelLayout>* cur_layout_ = nullptr;
    bool retained_ = false;               // the page being processed stays readable until its launches are confirmed
    int64_t resume_from_ = -1;            // set by a launcher that hands the rest of the page to another tier (see run_tiers)

    // ---- ungrouped tier (launch_global): one partial state per workgroup, merged into the state ----
    DevBuf slab_, state_;

    // ---- few-groups tier (launch_lds, confirm_*): the merge of page k runs on a second stream while the fused kernel of page k+1
    // streams.  Others only ask how many launches are unconfirmed (inflight.size()), read launch_seq (release_checkpoint) and
    // wait for the merges (drain_merges) ----
    struct LdsTier {
        DevBuf slab[2], entry_slot[2];
        hipStream_t merge_stream = nullptr;
        hipEvent_t ev_main[2] = {nullptr, nullptr}, ev_merge[2] = {nullptr, nullptr};
        bool merge_pending[2] = {false, false};
        int page = 0;
        bool probed = false;
        const Compiled* compiled = nullptr;  // the few-groups kernel in use (its lds_verdict is this plan's memory between operators)
        std::deque<Inflight> inflight;       // launches not confirmed yet (at most kMaxInflight)
        uint64_t launch_seq = 0;
    } lds_;

    // ---- the HBM table (op_fused_table.cpp; launch_table and launch_lds's merges fill it, op_fused_output.cpp reads it) ----
    struct HbmTable {
        DevBuf tag, keys, words, rep_count, spill[2];
        PinnedBuf h_rep;
        uint32_t cap = 0, rep = 1;
        // after a launch: groups_upper = the fullest replica (what every replica must have room for), groups_sum = upper bound of the
        // distinct groups
        uint64_t groups_upper = 0, groups_sum = 0;
        uint64_t probed_groups = 0;       // groups a probe launch saw before its table was given up (drop_table)
        bool probed = false;              // the launch that tells the cardinality has run
    } gt_;
    // ... indexed by build position instead (V_BROW, run_page_build_rows)
    bool build_rows_table_ = false;
    const Compiled* brow_keys_ = nullptr;  // its pa_brow_keys kernel
    int brow_occ_word_ = -1;               // KernelInfo::occ_word / occ_empty of the table
    uint64_t brow_occ_empty_ = 0;

    // ---- the hash-partitioned path and its partition-owned tables (V_LDSP): partitioned_wanted, run_page_partitioned; launch_table
    // passes the tables to the kernel, build_output folds them into the HBM table ----
    struct Partitioned {
        int parts = 0, lc = 0;            // partition-owned tables exist: their number, slots per table
        bool want = false;
        bool fresh = false;               // the partitions' tables exist but no launch has written them yet
        uint64_t fell = 0;                // rows that fell through to the HBM table (their partition's table was full)
        DevBuf tag, keys, words, count, part_first;
        DevBuf part_ids, part_pos, part_counts, part_temp;
        std::vector<DevBuf> reorder_bufs; // per channel: values, NULL flags of the partition-ordered copy of a chunk
        int list_grid_hint = 0;
    } ldsp_;

    // ---- interning and ranks (op_fused_intern.cpp) ----
    std::vector<std::unique_ptr<StringInterner>> interners_;  // per input channel, for Spec::interned channels
    PageStager dict_stager_;
    std::vector<DevBuf> dict_key_bufs_;  // per interned channel: uploaded ids, key ids, key NULL flags of a dictionary page
    std::vector<std::unique_ptr<RankedChannel>> ranked_;

    // ---- the eager result and the operator's last event (op_fused_output.cpp) ----
    struct Eager {
        bool on = true;          // PRESTO_AMD_EAGER_OUTPUT
        bool queued = false;     // finish() has enqueued the result; event, recorded behind it, says when it has landed
        hipEvent_t event = nullptr;
        bool with_state = false;  // the ungrouped state was copied behind the control block
        size_t rows = 0;         // ... or this many dense rows of keys, then of words (0: the table did not exist)
        uint64_t begun = 0;      // timer.begun() at finish: a launch after it (a redo at confirmation) voids the result
        PinnedBuf land;          // [0..31] control block, then the state words, or kEagerGroups rows of keys and of words
    } eager_;
    // Recorded on the main stream behind everything the operator has enqueued there, by every path that enqueues after the last
    // add_input (finish -- again behind an eager result that went to the main stream --, get_output's legacy path, emit_states);
    // last_valid_ is false from the first enqueue until it is recorded, and again after a redo at confirmation.  The destructor waits for it -- and, through pool_stream_release, for the merge stream, the eager result's copies on it
    // included -- before the members' destructors hand the pooled buffers back: that wait is what keeps a buffer out of the pool
    // while this operator's work still uses it.
    hipEvent_t last_event_ = nullptr;
    bool last_valid_ = false;  // (the constructor already enqueues: the control block's memset)

    // ---- the result page (op_fused_output.cpp) ----
    PinnedBuf h_table_, h_parts_;
    DevBuf dense_keys_, dense_words_, null_flags_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> out_storage_;
    int32_t out_rows_ = 0;
    // host copies of small key dictionaries (build_output's host assembly of a few groups)
    static constexpr int64_t kHostDecodeGroups = 4096;
    static constexpr uint32_t kHostDecodeIds = 4096;
    std::vector<std::vector<std::string>> host_dict_;
};

}  // namespace fused_op
}  // namespace pa
