// row_sort.hpp -- a row permutation sorted by (group id, sort channels) on device: the order of SimplePageWithPositionComparator inside
// each group, groups by ascending id, rows that compare equal in arrival (= array) order.
//
// The one row sort of OrderBy, TopNRanking and Window: a stable least-significant-digit sort of the permutation, channels from the last
// to the first.  A channel is turned into order-preserving 64-bit images (topn_kernels.hpp: integers, DATE, BOOLEAN, DOUBLE in
// Double.compare order; a VARCHAR as its 8-byte chunks, zero padded, with the length as the least significant key -- Slice.compareTo:
// unsigned bytes, a proper prefix sorts first), and the (image, row) PAIRS are sorted by the bits in which the images differ at all (OR /
// AND of the images, one read-back: keys below 2^40 are sorted by 40 bits, not 64 -- launch_sort_pairs, sort_kernels.hip); the images are
// brought into the current order by one gather first.  NULL rows get one constant image, and the channel's one-bit NULL digit above the
// images (NULLS FIRST / LAST, independent of ASC / DESC) is a stable two-way partition.  Then one more pair sort by the group ids.  The
// permutation is not written while it is still 0, 1, 2, ...: the first sort takes the row ids as implied.
//
// A SortCarry (OrderBy's) asks for what the first channel's pair sort can leave behind besides the permutation.
#pragma once

#include <vector>

#include "device_page.hpp"
#include "scan_kernels.hpp"
#include "sort_kernels.hpp"
#include "topn_kernels.hpp"

namespace pa {

struct SortCarry {
    SortPayload payload;                      // in: columns that may ride with the FIRST channel's pair sort (count 0: none) instead of being gathered
                                              //     through the permutation afterwards; the in / out arrays are the caller's.  They ride when that channel
                                              //     is fixed-width without NULL rows (no NULL digit follows) and its sort starts from the identity
    bool moved = false;                       // out: payload.out holds the columns in sorted order (the sort was PA_SORT_BUCKETS; the library's moves none)
    const uint64_t* sorted_images = nullptr;  // out: the first channel's images in sorted order, when its pair sort was the last thing that moved the
                                              //      permutation (null also when every image was equal).  Valid until the next sort() / release()
    int path = PA_SORT_NONE;                  // out: what the last image sort that ran returned (PA_SORT_BUCKETS / PA_SORT_LIBRARY)
};

class RowSorter {
public:
    // cols / orders: the sort channels (pa_sort_order) over n rows, VARCHAR offsets starting at 0; gids (may be null): n group ids below
    // 2^gid_bits, sorted by last so that they lead.  Returns the permutation (sorted index -> row), valid until the next call or release().
    const int32_t* sort(const std::vector<DevColumn>& cols, const std::vector<int32_t>& orders, const uint64_t* gids, int gid_bits, int64_t n, hipStream_t s,
                        SortCarry* carry = nullptr)
    {
        PA_REQUIRE(carry == nullptr || gids == nullptr, PA_ERR_ILLEGAL_STATE, "RowSorter: a carry cannot outlive the sort by group ids");
        carry_ = carry;
        if (carry) {
            carry->moved = false;
            carry->sorted_images = nullptr;
            carry->path = PA_SORT_NONE;
        }
        perm_ = static_cast<int32_t*>(perm_buf_[0].ensure((size_t)n * 4));
        next_ = static_cast<int32_t*>(perm_buf_[1].ensure((size_t)n * 4));
        pos_ = static_cast<int32_t*>(pos_buf_.ensure((size_t)n * 4));
        kp_[0] = static_cast<uint64_t*>(pair_keys_[0].ensure((size_t)n * 8));
        kp_[1] = static_cast<uint64_t*>(pair_keys_[1].ensure((size_t)n * 8));
        sort_temp_bytes_ = sort_pairs_temp_bytes(n, carry ? carry->payload.count : 0);
        sort_temp_ = radix_temp_.ensure(sort_temp_bytes_);
        or_and_ = static_cast<uint64_t*>(or_and_buf_.ensure(key_or_and_bytes()));
        h_or_and_.resize(key_or_and_bytes() / 8);
        int64_t* counts = static_cast<int64_t*>(counts_.ensure(256 * 8));
        uint64_t* keys = static_cast<uint64_t*>(keys_.ensure((size_t)n * 8));
        n_ = n;
        identity_ = true;   // the permutation is still 0, 1, 2, ...: not written until somebody needs it
        for (int i = (int)cols.size() - 1; i >= 0; i--) {
            const DevColumn& a = cols[(size_t)i];
            const bool descending = orders[(size_t)i] >= 2, nulls_first = (orders[(size_t)i] & 1) == 0;
            if (a.varwidth) {
                // least significant first: the length, then the 8-byte chunks from the last to the first
                const int32_t max_len = varchar_max_length(a.offsets, n, counts, s);
                const int chunks = (max_len + 7) / 8;
                for (int chunk = chunks; chunk >= 0; chunk--) {
                    launch_varchar_chunk_keys(a.values, a.offsets, a.nulls, n, chunk == chunks ? -1 : chunk, descending ? 1 : 0, keys, s);
                    sort_by_image(keys, 0, chunk != chunks, false, s);   // (the length key spreads; the byte chunks do not)
                }
            }
            else {
                // NULL rows get one constant image; their place relative to the values is decided by the NULL digit below
                const int pairs = launch_topn_keys_or_and(a.type, a.values, nullptr, a.nulls, n, descending ? PA_DESC_NULLS_LAST : PA_ASC_NULLS_LAST, keys, or_and_, s);
                sort_by_image(keys, pairs, a.type == PA_DOUBLE || a.type == PA_REAL, i == 0 && a.nulls == nullptr, s);
            }
            if (a.nulls) {
                int32_t* digits = static_cast<int32_t*>(digits_.ensure((size_t)n * 4));
                void* temp = part_temp_.ensure(partition_temp_bytes(n, 256));
                materialize(s);
                launch_sort_null_digits(a.nulls, perm_, n, nulls_first ? 1 : 0, digits, s);
                // one stable radix pass: rows grouped by digit, the current order kept inside a digit; perm' = perm o pos
                launch_partition_positions(digits, n, 2, pos_, counts, temp, s);
                launch_gather_flat(perm_, 4, pos_, n, next_, s);
                std::swap(perm_, next_);
                if (carry) carry->sorted_images = nullptr;
            }
        }
        if (gids != nullptr && gid_bits > 0) sort_pairs(gids, 0, gid_bits, false, s);
        materialize(s);   // (no sort ran: every image the same)
        return perm_;
    }

    void release()
    {
        for (DevBuf* b : {&perm_buf_[0], &perm_buf_[1], &digits_, &pos_buf_, &counts_, &keys_, &part_temp_, &pair_keys_[0], &pair_keys_[1], &radix_temp_, &or_and_buf_})
            b->release();
    }
    size_t bytes() const
    {
        return perm_buf_[0].capacity() + perm_buf_[1].capacity() + digits_.capacity() + pos_buf_.capacity() + counts_.capacity() + keys_.capacity() +
               part_temp_.capacity() + pair_keys_[0].capacity() + pair_keys_[1].capacity() + radix_temp_.capacity() + or_and_buf_.capacity();
    }

private:
    void materialize(hipStream_t s)
    {
        if (identity_) launch_iota_i32(perm_, n_, s);
        identity_ = false;
    }
    // pairs: OR / AND of the images already in or_and_ (the image kernel left them there), 0 = still to be computed
    // crowded: images of doubles (exponent bits) or text crowd under few bit prefixes -- the sort takes its bucket bounds from a sample
    // rides: the carry's payload may go with this sort (the first channel's, no NULL digit behind it)
    void sort_by_image(const uint64_t* keys, int pairs, bool crowded, bool rides, hipStream_t s)
    {
        if (carry_) carry_->sorted_images = nullptr;
        const uint64_t* in = keys;
        if (!identity_) {
            launch_gather_flat(keys, 8, perm_, n_, kp_[0], s);
            in = kp_[0];
        }
        const int blocks = pairs > 0 ? pairs : launch_key_or_and(in, n_, or_and_, s);
        read_back(h_or_and_.data(), or_and_, (size_t)blocks * 16, s);
        uint64_t h[2] = {0ULL, ~0ULL};
        for (int b = 0; b < blocks; b++) {
            h[0] |= h_or_and_[2 * (size_t)b];
            h[1] &= h_or_and_[2 * (size_t)b + 1];
        }
        const uint64_t varying = h[0] ^ h[1];
        if (varying == 0ULL) return;   // every image the same: the order stays
        int begin_bit = __builtin_ctzll(varying);
        const int end_bit = 64 - __builtin_clzll(varying);
        // (rocPRIM 4.0's merge-sort path for small inputs builds its mask of the bit range with 1 << end_bit: a range that ends at bit 64
        // without starting at bit 0 compares nothing -- such ranges are widened to the whole key)
        if (end_bit == 64) begin_bit = 0;
        sort_sorted_input(in, begin_bit, end_bit, crowded, rides, s);
    }
    // keys in row order (the group ids): brought into the current order, then sorted over [begin_bit, end_bit)
    void sort_pairs(const uint64_t* keys, int begin_bit, int end_bit, bool crowded, hipStream_t s)
    {
        const uint64_t* in = keys;
        if (!identity_) {
            launch_gather_flat(keys, 8, perm_, n_, kp_[0], s);
            in = kp_[0];
        }
        sort_sorted_input(in, begin_bit, end_bit, crowded, false, s);
    }
    void sort_sorted_input(const uint64_t* in, int begin_bit, int end_bit, bool crowded, bool rides, hipStream_t s)
    {
        const SortPayload* payload = rides && identity_ && carry_ && carry_->payload.count > 0 ? &carry_->payload : nullptr;
        const int path = launch_sort_pairs(in, identity_ ? nullptr : perm_, pos_, kp_[1], next_, n_, begin_bit, end_bit, sort_temp_, sort_temp_bytes_, s, payload,
                                           crowded ? PA_SORT_HINT_CROWDED : PA_SORT_HINT_SPREAD);
        std::swap(perm_, next_);
        identity_ = false;
        if (carry_) {
            carry_->moved = payload != nullptr && path == PA_SORT_BUCKETS;
            carry_->sorted_images = kp_[1];
            carry_->path = path;
        }
    }

    DevBuf perm_buf_[2], digits_, pos_buf_, counts_, keys_, part_temp_, pair_keys_[2], radix_temp_, or_and_buf_;
    std::vector<uint64_t> h_or_and_;
    int32_t* perm_ = nullptr;
    int32_t* next_ = nullptr;
    int32_t* pos_ = nullptr;
    uint64_t* kp_[2] = {nullptr, nullptr};
    uint64_t* or_and_ = nullptr;
    void* sort_temp_ = nullptr;
    size_t sort_temp_bytes_ = 0;
    int64_t n_ = 0;
    bool identity_ = true;
    SortCarry* carry_ = nullptr;   // of the sort() that is running
};

}  // namespace pa
