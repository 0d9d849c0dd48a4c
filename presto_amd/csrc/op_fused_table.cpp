// op_fused_table.cpp -- FusedAggregationOperator (op_fused.hpp): the HBM group table -- sizing, replicas, folding, the group counts read
// back after a launch -- and the hash-partitioned path that runs the LDS-table kernels over it (partitioned_wanted,
// run_page_partitioned: hash-partitioned LDS tables, partition-owned tables).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "op_fused.hpp"

namespace pa {
namespace fused_op {

// replicas wanted for a table of g groups: enough distinct accumulator addresses (>= ~2^17) for the atomics of a
// launch not to queue on a few of them; none needed once the groups themselves are that many
uint32_t FusedAggregationOperator::desired_replicas(uint64_t g)
{
    uint64_t r = (1ULL << 17) / std::max<uint64_t>(g, 1);
    uint32_t p = 1;
    while (p * 2 <= r && p < 128) p <<= 1;
    return p;
}

// makes room for at least min_groups groups per replica at a load factor of one half; reps = 0 keeps the replica count
void FusedAggregationOperator::ensure_table(uint64_t min_groups, uint32_t reps)
{
    if (reps == 0) reps = gt_.rep;
    if (reps < gt_.rep) min_groups = std::max(min_groups, gt_.groups_sum);  // replicas fold into fewer tables
    uint64_t want = std::max<uint64_t>(1024, 2 * min_groups);
    PA_REQUIRE(want <= (1ULL << 30), PA_ERR_INSUFFICIENT_RESOURCES, "Size of hash table cannot exceed 1 billion entries");
    uint32_t cap = std::max(next_pow2(want), gt_.cap);
    const size_t slot_bytes = 8 * (size_t)(1 + std::max(w_, 1) + nw_);
    while (reps > 1 && (size_t)reps * cap * slot_bytes > (8ULL << 30)) reps >>= 1;
    if (cap == gt_.cap && reps == gt_.rep) return;
    hipStream_t s = stream_.get();
    drain_merges();  // in-flight merges still write the old table
    DevBuf tag, keys, words, rc;
    const size_t slots = (size_t)reps * cap;
    tag.ensure(slots * 8);
    keys.ensure(slots * 8 * std::max(w_, 1));
    words.ensure(slots * 8 * nw_);
    rc.ensure(128 * 4);
    PA_HIP(hipMemsetAsync(tag.ptr(), 0, slots * 8, s));
    // (PA_GT_KEY_CLEAR: no slot's key words may look like a key before the slot is claimed -- see pa_gt_upsert_n's fast path)
    PA_HIP(hipMemsetAsync(keys.ptr(), 0xA5, slots * 8 * std::max(w_, 1), s));
    PA_HIP(hipMemsetAsync(words.ptr(), 0, slots * 8 * nw_, s));
    PA_HIP(hipMemsetAsync(rc.ptr(), 0, 128 * 4, s));
    if (gt_.cap > 0) {
        PA_REQUIRE(kinds_dev_ != nullptr, PA_ERR_ILLEGAL_STATE, "group table without a compiled kernel");
        PA_HIP(hipMemsetAsync(ctl_ + 1, 0, 4, s));
        launch_gt_fold(gt_.tag.as<uint64_t>(), gt_.keys.as<uint64_t>(), gt_.words.as<uint64_t>(), gt_.cap, gt_.rep, std::max(w_, 1), nw_,
                       kinds_dev_, tag.as<uint64_t>(), keys.as<uint64_t>(), words.as<uint64_t>(), cap - 1, reps, ctl_ + 1,
                       rc.as<int32_t>(), ctl_, s);
        PA_HIP(hipStreamSynchronize(s));  // the old arrays return to the pool below
    }
    gt_.tag = std::move(tag);
    gt_.keys = std::move(keys);
    gt_.words = std::move(words);
    gt_.rep_count = std::move(rc);
    gt_.cap = cap;
    gt_.rep = reps;
}

// Groups of the whole input, from the d distinct keys among the first n rows, as if the keys were drawn uniformly from G
// values: d = G (1 - exp(-n / G)).  (Skewed keys make it an overestimate; it only ever chooses between tiers.)
uint64_t FusedAggregationOperator::estimate_groups(uint64_t d, uint64_t n)
{
    if (d == 0 || n == 0 || d * 8 < n) return d;  // most rows repeat a key already seen: d is about all there is
    if (d * 100 >= n * 98) return 32 * n;         // nearly every row a new key: "many" is all that can be said
    double lo = (double)d, hi = 64.0 * (double)n;
    for (int i = 0; i < 60; i++) {
        const double g = 0.5 * (lo + hi);
        if (g * (1.0 - std::exp(-(double)n / g)) < (double)d) lo = g;
        else hi = g;
    }
    return (uint64_t)hi;
}

// the HBM table and everything in it is given up (see lone_probe)
void FusedAggregationOperator::drop_table()
{
    hipStream_t s = stream_.get();
    drain_merges();
    gt_.tag.release();
    gt_.keys.release();
    gt_.words.release();
    gt_.rep_count.release();
    gt_.cap = 0;
    gt_.rep = 1;
    PA_HIP(hipMemsetAsync(ctl_ + 1, 0, 4, s));
    gt_.groups_upper = gt_.groups_sum = 0;
}

// group counts of all replicas after a launch: gt_.groups_upper = the fullest replica (what every replica must have
// room for), gt_.groups_sum = upper bound of the distinct groups
void FusedAggregationOperator::read_group_counts(hipStream_t s)
{
    int32_t* h = static_cast<int32_t*>(gt_.h_rep.ensure(128 * 4));
    h[0] = 0;
    if (gt_.rep > 1) PA_HIP(hipMemcpyAsync(h, gt_.rep_count.ptr(), (size_t)gt_.rep * 4, hipMemcpyDeviceToHost, s));
    PA_HIP(hipMemcpyAsync(h_ctl_, ctl_, 32, hipMemcpyDeviceToHost, s));
    PA_HIP(hipStreamSynchronize(s));
    uint64_t mx = (uint64_t)h_ctl_[1], sum = (uint64_t)h_ctl_[1];
    for (uint32_t r = 1; r < gt_.rep; r++) {
        mx = std::max<uint64_t>(mx, (uint64_t)h[r]);
        sum += (uint64_t)h[r];
    }
    gt_.groups_upper = mx;
    gt_.groups_sum = sum;
}

void FusedAggregationOperator::drain_merges()
{
    if (lds_.merge_stream) PA_HIP(hipStreamSynchronize(lds_.merge_stream));
    lds_.merge_pending[0] = lds_.merge_pending[1] = false;
}

// Medium cardinality on the HBM-table tier (G groups, lc / 2 < G <= 8 K): partition the rows by hash(key) mod P so that
// a partition holds ~lc / 8 groups, then run the LDS-table kernel over the rows in partition order, one contiguous slice
// per workgroup -- the atomics per row move from HBM (~20 G/s for the whole chip) into LDS.
bool FusedAggregationOperator::partitioned_wanted(const std::string& sig, const std::vector<ChannelLayout>& layout, int* partitions)
{
    if (getenv("PRESTO_AMD_NO_PARTITIONED")) return false;
    if (spec_.join) return false;  // a row's partition would need its probe: the row function runs once per row behind a probe stage
    if (spec_.any_ranked()) return false;  // (re-ranking walks the HBM table)
    if (ldsp_.parts > 0) {  // partition-owned tables exist: every later page is cut the same way
        *partitions = ldsp_.parts;
        return true;
    }
    static const uint64_t ldsp_from = [] {
        const char* e = getenv("PRESTO_AMD_LDSP_FROM");
        return (uint64_t)(e ? atoll(e) : 200000);
    }();
    const uint64_t expected = (uint64_t)std::max(spec_.expected_groups, 0);
    // nothing measured yet: only the planner's estimate can name the tier -- when it says "many groups", start with the
    // partition-owned tables at once (a probe launch on the HBM table would leave its groups there, to be folded later)
    if (!gt_.probed && (expected < ldsp_from || is_combiner_)) return false;
    // measured (64 M rows, 16 B/row, uniform keys; steady state per page): 1 K groups 9 -> 26 G rows/s, 8 K 6 -> 18 G,
    // 100 K 8 -> 11.6 G; beyond ~400 K groups a workgroup's slice holds more groups than its table takes
    const uint64_t g = std::max(gt_.groups_upper, gt_.probed_groups);
    const uint64_t g_est = std::max(g, expected);
    if (g_est < 256) return false;
    const Compiled* ldsh = nullptr;
    try {
        ldsh = &kernel_for(sig, layout, V_LDSH);
    }
    catch (const Error& e) {
        if (e.code != PA_ERR_NOT_SUPPORTED) throw;
        return false;
    }
    // Many groups: partition-owned tables (V_LDSP).  With the workgroup's table flushed into the HBM table after every
    // launch, a launch costs one HBM upsert per (group, launch) -- at 3 M groups and 2^24-row pages as many atomics as
    // rows / 5, and the tier stays bound by them (9 G rows/s).  A table that belongs to ONE partition for good is loaded
    // from and stored to HBM with plain coalesced accesses instead.  Partitions sized for ~0.4 of a table (they may fill to
    // 3/4 before rows fall through to the HBM table), from what the probe saw or the planner expects, whichever is more.
    if (g_est >= ldsp_from && g_est <= 2048ULL * (uint64_t)ldsh->info.lc * 3 / 4) {
        uint64_t p = next_pow2((uint64_t)((double)g_est / (0.4 * ldsh->info.lc)) + 1);
        *partitions = (int)std::min<uint64_t>(std::max<uint64_t>(p, 64), 2048);
        ldsp_.want = true;
        return true;
    }
    if (!gt_.probed || g < 256) return false;
    const uint64_t per = std::max(ldsh->info.lc / 8, 8);
    // at most 512 partitions (+ 1 for filtered rows), each within a quarter of the workgroup's table
    // up to half a table per partition (with one workgroup per partition, see ldsp_.list_grid_hint): 700 K groups 17 vs 10 G rows/s
    // on the HBM table, 1 M groups even
    // (beyond that the HBM table takes the rows as they come: running ITS kernel over partition-ordered rows, for the
    // locality of the table slice, was measured slower -- 3 M groups 7.2 vs 9.5 G rows/s, 10 M 6.1 vs 7.8: the atomics are
    // bound in the L2 atomic units, not by where the table lines live)
    // (The multisplit takes up to 4096 partitions in one pass, but more than 512 here was measured slower: with the table
    // flushed into HBM after every launch, 2048 partitions of a 2^24-row page are 8 K-row slices whose table set-up and
    // flush outweigh the rows -- 700 K groups 17.6 -> 11.8 G rows/s; the partition-owned tables above take over instead.)
    static const uint64_t max_parts = [] {
        const char* e = getenv("PRESTO_AMD_MAX_PARTITIONS");
        return (uint64_t)(e ? std::max(atoi(e), 2) : 512);
    }();
    if (g > max_parts * (uint64_t)(ldsh->info.lc / 2)) return false;
    uint64_t p = next_pow2((g + per - 1) / per);
    *partitions = (int)std::min<uint64_t>(std::max<uint64_t>(p, 2), max_parts);
    return true;
}

void FusedAggregationOperator::run_page_partitioned(const std::string& sig, const std::vector<ChannelLayout>& layout, const DevPage& dp, bool vec, int partitions,
                          int64_t start_row)
{
    hipStream_t s = stream_.get();
    // (A variant that also wrote every row's packed key / input words, put them in partition order and let the kernel read
    // them contiguously was measured slower at every cardinality -- 8 K groups 14.8 vs 17.9 G rows/s, 100 K 10.5 vs 11.6 --
    // than letting the LDS-table kernel gather the page rows of its slice, and was removed.)
    const Compiled& hk = kernel_for(sig, layout, V_HASH);
    bool ldsp = ldsp_.want || ldsp_.parts > 0;
    // (needs the reordered columns: fixed-width inputs, few enough for one multisplit)
    int moved = 0;
    for (int c = 0; c < spec_.n_in && ldsp; c++) {
        if (!spec_.used_channel[c]) continue;
        // (the multisplit moves 1-, 4- and 8-byte elements: a LONG_DECIMAL input keeps the position list, as a VARCHAR one does)
        ldsp = !dp.cols[c].varwidth && type_width(dp.cols[c].type) <= 8;
        moved += 1 + (dp.cols[c].nulls ? 1 : 0);
    }
    ldsp = ldsp && moved <= kMsplitMaxCols && !getenv("PRESTO_AMD_NO_MSPLIT");
    if (!ldsp && ldsp_.parts == 0) ldsp_.want = false;
    if (!ldsp) partitions = std::min(partitions, 512);  // (the position list is made for at most 512 partitions + 1 for the filtered rows)
    const Compiled& lk = kernel_for(sig, layout, ldsp ? V_LDSP : V_LDSH);
    cur_sig_ = &sig;
    cur_layout_ = &layout;
    if (ldsp && ldsp_.parts == 0) {
        // the partitions' tables, all empty
        ldsp_.parts = partitions;
        const size_t slots = (size_t)partitions * lk.info.lc;
        // (not cleared: the first launch starts every partition's table from zeroes in LDS and stores all of them)
        ldsp_.tag.ensure(slots * 8);
        ldsp_.keys.ensure(slots * 8 * std::max(lk.info.w, 1));
        ldsp_.words.ensure(slots * 8 * lk.info.nw);
        ldsp_.count.ensure((size_t)partitions * 4);
        ldsp_.lc = lk.info.lc;
        ldsp_.fresh = true;
    }
    if (ldsp) partitions = ldsp_.parts;
    const int64_t chunk = (int64_t)1 << 26;
    for (int64_t offset = start_row; offset < dp.n; offset += chunk) {
        const int64_t n = std::min(chunk, dp.n - offset);
        PaFusedArgs a;
        memset(&a, 0, sizeof a);
        for (int c = 0; c < spec_.n_in; c++) {
            if (!spec_.used_channel[c]) continue;
            const DevColumn& col = dp.cols[c];
            a.v[c] = col.varwidth ? col.values : static_cast<const char*>(col.values) + offset * type_width(col.type);
            a.o[c] = col.offsets ? col.offsets + offset : nullptr;
            a.nl[c] = col.nulls ? col.nulls + offset : nullptr;
        }
        a.n = n;
        a.vec = (vec && offset % 4 == 0) ? 1 : 0;
        a.err = ctl_;
        a.part_ids = static_cast<int32_t*>(ldsp_.part_ids.ensure((size_t)n * 4));
        a.part_mask = (uint32_t)partitions - 1;
        // the partition pass leaves the multisplit's tile x partition counts behind (tile-major, in the multisplit's scratch)
        void* ms_temp = ldsp_.part_temp.ensure(std::max(msplit_temp_bytes(n, partitions + 1), partition_temp_bytes(n, partitions + 1)));
        a.sub_count = msplit_counts(ms_temp);
        void* params[] = {&a};
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(msplit_tiles(n), (int64_t)cus_ * 8));
        timer.begin(s);
        PA_HIP(hipModuleLaunchKernel(hk.kernel.fn, grid, 1, 1, hk.info.block, 1, 1, 0, s, params, nullptr));
        int64_t* counts = static_cast<int64_t*>(ldsp_.part_counts.ensure((size_t)(partitions + 1) * 8));
        // (pays only when a slice of two partitions would overfill the table -- 500 K groups: 15 -> 20 G rows/s; below that
        // the second round of workgroups costs more than the sparser tables save -- 300 K: 24.7 -> 22.9)
        ldsp_.list_grid_hint = (2 * gt_.groups_upper / (uint64_t)partitions > (uint64_t)lk.info.lc * 3 / 8) ? partitions : 0;
        // fixed-width inputs: the used columns themselves are regrouped by partition (LDS-staged multisplit, coalesced both
        // ways) and the LDS-table kernel reads its slice contiguously; with a position list it pays a cache line per row
        // and column.  VARCHAR inputs keep the position list.
        bool reorder = !getenv("PRESTO_AMD_NO_MSPLIT");
        for (int c = 0; c < spec_.n_in && reorder; c++) reorder = !spec_.used_channel[c] || (!dp.cols[c].varwidth && type_width(dp.cols[c].type) <= 8);
        if (reorder) {
            std::vector<MsplitCol> mc;
            DevPage rp;
            rp.cols.resize(spec_.n_in);
            if (ldsp_.reorder_bufs.empty()) ldsp_.reorder_bufs.resize((size_t)spec_.n_in * 2);
            for (int c = 0; c < spec_.n_in; c++) {
                if (!spec_.used_channel[c]) continue;
                const DevColumn& col = dp.cols[c];
                const int w = type_width(col.type);
                DevColumn& out = rp.cols[c];
                out.type = col.type;
                out.values = ldsp_.reorder_bufs[(size_t)c * 2].ensure((size_t)n * w);
                mc.push_back(MsplitCol{static_cast<const char*>(col.values) + offset * w, const_cast<void*>(out.values), w, 0});
                if (col.nulls) {
                    out.nulls = static_cast<const uint8_t*>(ldsp_.reorder_bufs[(size_t)c * 2 + 1].ensure((size_t)n));
                    mc.push_back(MsplitCol{col.nulls + offset, const_cast<uint8_t*>(out.nulls), 1, 0});
                }
            }
            reorder = mc.size() <= (size_t)kMsplitMaxCols;
            if (reorder) {
                launch_msplit(a.part_ids, n, partitions + 1, mc.data(), (int32_t)mc.size(), counts, ms_temp, s, false, true);
                if (ldsp) {
                    // the kernel finds its rows through the partition boundaries on the device: the host does not need them
                    launch_exclusive_prefix_i64(counts, partitions + 1, static_cast<int64_t*>(ldsp_.part_first.ensure((size_t)(partitions + 2) * 8)), s);
                    timer.end(s, false);
                    rp.n = (int32_t)n;
                    RowList list{nullptr, n, 0, n};
                    run_page(lk, rp, false, &list);
                    continue;
                }
                timer.end(s, false);
                int64_t dropped = 0;
                PA_HIP(hipMemcpyAsync(&dropped, counts + partitions, 8, hipMemcpyDeviceToHost, s));
                PA_HIP(hipStreamSynchronize(s));
                rp.n = (int32_t)(n - dropped);  // the filtered rows are the last partition
                RowList list{nullptr, n - dropped, 0, n - dropped};
                if (list.count > 0) run_page(lk, rp, false, &list);
                continue;
            }
        }
        int32_t* positions = static_cast<int32_t*>(ldsp_.part_pos.ensure((size_t)n * 4));
        launch_partition_positions(a.part_ids, n, partitions + 1, positions, counts, ms_temp, s);
        timer.end(s, false);
        int64_t dropped = 0;
        PA_HIP(hipMemcpyAsync(&dropped, counts + partitions, 8, hipMemcpyDeviceToHost, s));
        PA_HIP(hipStreamSynchronize(s));
        RowList list{positions, n - dropped, offset, n};
        if (list.count > 0) run_page(lk, dp, vec, &list);
    }
}

}  // namespace fused_op
}  // namespace pa
