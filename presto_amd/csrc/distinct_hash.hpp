// distinct_hash.hpp -- what the operators over GroupByHash.getGroupIds share (op_distinct.cpp, op_row_number.cpp): the growing key table
// of distinct_kernels.hpp with its key store and string interners.
#pragma once

#include <algorithm>
#include <deque>
#include <memory>
#include <vector>

#include "device_page.hpp"
#include "distinct_kernels.hpp"
#include "intern_kernels.hpp"
#include "scan_kernels.hpp"

namespace pa {

constexpr int32_t kDefaultExpectedDistinct = 10000;   // the reference's expectedGroups when the planner gives none
constexpr int64_t kMaxDistinct = (int64_t)1 << 30;    // table of 2^31 slots at most (BigintGroupByHash.java:264-267 stops there too)

inline uint32_t pow2_at_least(int64_t v)
{
    uint32_t p = 16;
    while ((int64_t)p < v) p <<= 1;
    return p;
}

// The keys seen so far: slot table, key store, one StringInterner per VARCHAR channel.  Not thread safe (one operator, one driver thread).
class DistinctHash {
public:
    DistinctHash(const std::vector<int32_t>& key_types, int32_t expected, hipStream_t s) : types_(key_types)
    {
        interners_.resize(types_.size());
        for (size_t c = 0; c < types_.size(); c++)
            if (types_[c] == PA_VARCHAR) interners_[c].reset(new StringInterner());
        // two counter words {page sequence << 32 | distinct count} taken in turn, the page's new keys, the error flag
        words_ = static_cast<uint64_t*>(words_buf_.ensure(64));
        PA_HIP(hipMemsetAsync(words_, 0, 64, s));
        h_counter_ = static_cast<uint64_t*>(h_counter_buf_.ensure(64));
        *h_counter_ = 0;
        new_table(pow2_at_least(2 * (int64_t)(expected > 0 ? expected : kDefaultExpectedDistinct)), s);
    }

    // Passes 1 to 3 over the staged key columns of one page (n > 0).  mark: round_up(n, 4) bytes.  out_positions (may be null):
    // the positions of the first `limit` new keys, in order.  gids (may be null; n words): the group id of every row
    // (GroupByHash.getGroupIds) -- the insert pass then runs as its second instantiation, which also notes the slot every probe ended
    // at, and a gather behind the publish pass reads the ids out of those slots.  Returns the name of the timed kernel.
    const char* add_page(const DevColumn* const* cols, int32_t n, uint8_t* mark, int32_t* out_positions, int64_t limit, KernelTimer& timer, hipStream_t s,
                         uint64_t* gids = nullptr)
    {
        reserve(n, s);
        const size_t nc = types_.size();
        DistinctCanonArgs ca;
        memset(&ca, 0, sizeof ca);
        DistinctKeys keys;
        memset(&keys, 0, sizeof keys);
        bool any_nulls = false, any_out = false;
        for (size_t c = 0; c < nc; c++) {
            const DevColumn& col = *cols[c];
            PA_REQUIRE(col.type == types_[c], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared distinct channel type");
            any_nulls = any_nulls || col.nulls != nullptr;
            if (types_[c] == PA_VARCHAR) {
                // exact dense ids: byte equality of strings is integer equality of ids
                const int32_t* ids = interners_[c]->intern(col.values, col.offsets, col.nulls, n, s);
                ca.src[c] = JoinCol{ids, nullptr, col.nulls, PA_INTEGER, 0};
            }
            else if ((types_[c] == PA_BIGINT || types_[c] == PA_DECIMAL) && col.nulls == nullptr) {
                keys.words[c] = static_cast<const uint64_t*>(col.values);   // already canonical: read in place
                continue;
            }
            else ca.src[c] = JoinCol{col.values, nullptr, col.nulls, col.type, 0};
            ca.out[c] = static_cast<uint64_t*>(canon_[c].ensure((size_t)n * 8));
            keys.words[c] = ca.out[c];
            any_out = true;
        }
        keys.ncols = ca.ncols = (int32_t)nc;
        keys.n = ca.n = n;
        if (any_nulls) keys.nullbits = ca.nullbits = static_cast<uint8_t*>(nullbits_.ensure((size_t)n));
        if (any_nulls || any_out) launch_distinct_canon(ca, s);

        const size_t padded = ((size_t)n + 3) & ~(size_t)3;
        int32_t* slot_of = static_cast<int32_t*>(slot_of_.ensure(padded * 4));
        const int64_t blocks = distinct_blocks(n);
        int32_t* block_counts = static_cast<int32_t*>(block_counts_.ensure((size_t)blocks * 4));
        void* temp = scan_temp_.ensure(scan_temp_bytes(blocks));
        int32_t* page_total = reinterpret_cast<int32_t*>(words_ + 2);
        const DistinctStore store = store_view();
        const DistinctTable table{slots_.as<uint64_t>(), capacity_ - 1, 0};
        seq_++;
        DistinctPublishArgs pa;
        memset(&pa, 0, sizeof pa);
        pa.keys = keys;
        pa.store = store;
        pa.table = table;
        pa.slot_of = slot_of;
        pa.mark = mark;
        pa.block_offsets = block_counts;
        pa.page_total = page_total;
        pa.counter_in = words_ + ((seq_ & 1u) ^ 1u);
        pa.counter_out = words_ + (seq_ & 1u);
        pa.out_positions = out_positions;
        pa.err = reinterpret_cast<int32_t*>(words_ + 3);
        pa.limit = limit;
        pa.seq = seq_;
        int32_t* stop_of = gids != nullptr ? static_cast<int32_t*>(stop_of_.ensure((size_t)n * 4)) : nullptr;
        timer.begin(s);
        if (stop_of != nullptr) launch_distinct_insert_ids(keys, store, table, slot_of, stop_of, s);
        else launch_distinct_insert(keys, store, table, slot_of, s);
        launch_distinct_mark(table, slot_of, n, mark, block_counts, s);
        launch_exclusive_scan_i32(block_counts, block_counts, blocks, page_total, temp, s);
        launch_distinct_publish(pa, s);
        timer.end(s);
        // the count comes back behind the page without a wait (StringInterner::settle's way): bound() reads what has landed
        PA_HIP(hipMemcpyAsync(h_counter_, pa.counter_out, 8, hipMemcpyDeviceToHost, s));
        fed_.emplace_back(seq_, n);
        fed_rows_ += n;
        if (stop_of == nullptr) return "k_distinct_insert";
        launch_distinct_group_ids(table, stop_of, n, gids, s);
        return "k_distinct_insert_ids";
    }

    // nextDistinctId, exact: waits for the pages in flight
    int64_t settle(hipStream_t s)
    {
        if (!fed_.empty()) {
            PA_HIP(hipStreamSynchronize(s));
            bound();
            int32_t err = 0;
            read_back(&err, words_ + 3, 4, s);
            PA_REQUIRE(err == 0, PA_ERR_DEVICE, "distinct key store overrun");
        }
        return count_;
    }
    int64_t capacity() const { return capacity_; }
    int64_t memory_bytes() const
    {
        size_t b = slots_.capacity() + store_null_.capacity() + nullbits_.capacity() + slot_of_.capacity() + stop_of_.capacity() + block_counts_.capacity() +
                   scan_temp_.capacity();
        for (size_t c = 0; c < types_.size(); c++) {
            b += store_words_[c].capacity() + canon_[c].capacity();
            if (interners_[c]) b += interners_[c]->bytes();
        }
        return (int64_t)b;
    }

private:
    // an upper bound of the distinct count without a wait: the count of the last page whose counter has landed + the rows fed since
    int64_t bound()
    {
        const uint64_t landed = __atomic_load_n(h_counter_, __ATOMIC_ACQUIRE);
        const uint32_t seq = (uint32_t)(landed >> 32);
        count_ = (int64_t)(uint32_t)landed;
        while (!fed_.empty() && (int32_t)(seq - fed_.front().first) >= 0) {
            fed_rows_ -= fed_.front().second;
            fed_.pop_front();
        }
        return count_ + fed_rows_;
    }
    // room for n more keys in the table (load factor 1/2) and in the store
    void reserve(int32_t n, hipStream_t s)
    {
        int64_t need = bound() + n;
        if (2 * need <= (int64_t)capacity_ && need <= (int64_t)store_capacity_) return;
        need = settle(s) + n;
        PA_REQUIRE(need <= kMaxDistinct, PA_ERR_INSUFFICIENT_RESOURCES, "distinct table exceeds 2^30 keys");
        if (need > (int64_t)store_capacity_) {
            const int64_t cap = std::max<int64_t>(need, 2 * (int64_t)store_capacity_);
            for (size_t c = 0; c < types_.size(); c++) store_words_[c].reserve_keep((size_t)cap * 8, (size_t)count_ * 8, s);
            store_null_.reserve_keep((size_t)cap, (size_t)count_, s);
            store_capacity_ = (uint32_t)cap;
        }
        if (2 * need > (int64_t)capacity_) {
            new_table(pow2_at_least(2 * need), s);
            launch_distinct_rehash(store_view(), (int32_t)types_.size(), (uint32_t)count_, DistinctTable{slots_.as<uint64_t>(), capacity_ - 1, 0}, s);
        }
    }
    void new_table(uint32_t slots, hipStream_t s)
    {
        DevBuf fresh;
        void* p = fresh.ensure((size_t)slots * 8);
        PA_HIP(hipMemsetAsync(p, 0xff, (size_t)slots * 8, s));
        // (the old table goes back to the pool tagged with this stream: it is granted again only behind the work enqueued so far)
        slots_ = std::move(fresh);
        capacity_ = slots;
    }
    DistinctStore store_view()
    {
        DistinctStore st;
        memset(&st, 0, sizeof st);
        for (size_t c = 0; c < types_.size(); c++) st.words[c] = store_words_[c].as<uint64_t>();
        st.nullbits = store_null_.as<uint8_t>();
        st.capacity = store_capacity_;
        return st;
    }

    std::vector<int32_t> types_;
    std::vector<std::unique_ptr<StringInterner>> interners_;
    DevBuf slots_, store_words_[kMaxJoinChannels], store_null_, canon_[kMaxJoinChannels], nullbits_, slot_of_, stop_of_, block_counts_,
        scan_temp_, words_buf_;
    PinnedBuf h_counter_buf_;
    uint64_t* words_ = nullptr;
    uint64_t* h_counter_ = nullptr;
    uint32_t capacity_ = 0, store_capacity_ = 0, seq_ = 0;
    int64_t count_ = 0, fed_rows_ = 0;
    std::deque<std::pair<uint32_t, int32_t>> fed_;   // pages whose counter has not landed yet: {sequence number, rows}
};

}  // namespace pa
