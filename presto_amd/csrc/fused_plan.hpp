// fused_plan.hpp -- what the fused scan-filter-project(-probe)-aggregate operator is asked to do, in the form its code generator
// (fused_codegen.cpp + one fused_tier_*.cpp per kernel tier) and its host side (op_fused.hpp) share: the plan (Spec), the tiers
// (Variant) and what a generated kernel tells the host about itself (KernelInfo).  The kernels' argument block is PaFusedArgs
// (kernels/pa_args.h), the one definition the kernels and the host both use.
#pragma once

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "exprgen.hpp"
#include "operator.hpp"
#include "probe_stage.hpp"

namespace pa {
namespace fused {

// V_LDSP: the LDS-table variant with partition-owned tables (see PaFusedArgs::sub_tag)
// V_BROW: probe stage whose group keys are functions of the build row: the table slot is the build position
// V_GLOBAL_R / V_LDS_R: the ungrouped / few-groups kernels over a TABLE of row ranges (stable device pages that do not continue
// each other in memory, taken in place by one launch: see ranges_)
// V_GLOBAL_S: the ungrouped kernel whose page loop loads the columns of a staged plan (Spec::n_stages) only for the rows still alive
enum Variant { V_GLOBAL = 0, V_LDS = 1, V_GT = 2, V_LDSH = 3, V_HASH = 4, V_LDSP = 5, V_BROW = 6, V_GLOBAL_R = 7, V_LDS_R = 8, V_GLOBAL_S = 9 };
constexpr int kMaxStages = 4;
// rows per entry of a range table: one workgroup takes an entry at a time
constexpr int64_t kRangeRows = 8192, kRangeRowsLds = 4096;
enum WordKind { W_CNT = 0, W_SUMF = 1, W_SUMI = 2, W_MAXU = 3 };

constexpr int kLdsSlots = 8;  // C of the LDS variant: 8 groups x NW words x 64 lanes x 8 B of LDS per wave

// Group keys are bit-packed into as few 64-bit words as possible (Q1: two VARCHAR(1) keys -> one word).
struct KeyPart {
    int32_t type = PA_BIGINT;
    int word = 0;        // word holding the value (first of two for long VARCHAR)
    int shift = 0;       // bit offset inside the word
    int bits = 64;       // value bits (long VARCHAR: 128 = two dedicated words)
    int bound = 0;       // short VARCHAR: declared length bound (1..7)
    int null_word = -1;  // position of the IS NULL flag, or -1
    int null_shift = 0;
};

// The probe stage (probe_stage.hpp) between the projections and the aggregation; its build columns are those the aggregation reads.
struct JoinStage : ProbeStage {
    int key_proj = -1;                 // projection that is the probe join key
    // per group key: the projection to take it from when the slot is the build position (build columns only: the probe join key
    // is replaced by the build key column, equal on every match); empty = the group keys do not determine / are not determined
    // by the build row, no BROW variant
    std::vector<int> brow_group_proj;
};

struct Spec {
    std::shared_ptr<JoinStage> join;   // null: no probe stage
    // per channel: read inside the selected-rows block only (probe stage: everything the filter and the probe key do not need
    // is loaded for the rows that found a match, not for the whole page)
    std::vector<bool> lazy_channel;
    // Staged loads (no probe stage, a filter): the filter's top-level AND flattened into its conjuncts, in the written order
    // (node ids of `filter`), and per used channel the stage that loads it -- stage k evaluates conjuncts conjunct_begin[k] ..
    // conjunct_begin[k + 1] - 1 for the rows still alive and then asks for the channels of stage k + 1; the last stage loads what
    // only the projections read and accumulates.  n_stages < 2: no staging (channel_stage all 0 or -1 for unused channels).
    std::vector<int32_t> conjuncts;
    std::vector<int> conjunct_begin;  // per stage (n_stages entries; the last stage evaluates no conjunct when it is the projections')
    std::vector<int> channel_stage;   // per channel: -1 unused
    int n_stages = 0;
    int n_in = 0;
    std::vector<int32_t> in_types, in_params;
    bool has_filter = false;
    OwnedExpr filter;
    std::vector<OwnedExpr> proj;
    std::vector<int> group_proj;
    int hash_channel = -1;
    std::vector<pa_aggregate> aggs;
    int expected_groups = 0;
    int64_t max_partial_memory = 0;
    int step = PA_STEP_SINGLE;
    int output_mem = PA_MEM_HOST;
    std::vector<bool> used_channel;
    std::vector<int> short_bound;  // per channel: > 0 when the channel is a short VARCHAR group key (packed bytes passed as cs<c>)
    // per channel: VARCHAR group key of unknown or long (> 15 bytes) bound, replaced by its interned id before the kernels
    // see the page (intern_kernels.hpp); in_types / the projection's type say INTEGER for such a channel
    std::vector<bool> interned;
    // per channel: VARCHAR argument of min / max without a short bound.  The page's strings are interned and the kernels see a BIGINT
    // column in their place -- (rank of the string among the dictionary's strings) << 32 | id -- whose integer order is the strings'
    // order; the operator re-ranks what it accumulated whenever a page brings new strings (op_fused_intern.cpp: rank_values)
    std::vector<bool> ranked;
    bool any_ranked() const
    {
        for (bool r : ranked) if (r) return true;
        return false;
    }
    // channels the kernels do not read as they arrive
    bool derived(int c) const { return interned[c] || ranked[c]; }
};

struct KernelInfo {
    std::string source, entry;
    int variant = V_GLOBAL;
    bool ranged = false;  // the kernel walks a table of row ranges (V_GLOBAL_R / V_LDS_R; `variant` names the base variant)
    // V_GLOBAL_S: bytes per row each stage loads (values and NULL flags); the kernel writes, per workgroup, the rows that asked for
    // the columns of stage 1 .. n - 1 into slab words gridDim.x * nw + blockIdx.x * (n - 1) + k - 1 (the decision: op_fused_kernels.cpp, staged_decide)
    std::vector<int> stage_bytes;
    int nw = 0, w = 0, c = 0, block = 256;
    // the group key is "packed": one key word, of which the parts and their NULL flags use at most 31 bits.  The few-groups tier
    // then keeps its key table as 32-bit words whose empty value, 0xFFFFFFFF, no key can take (fused_tier_lds.cpp)
    bool packed_key = false;
    int lc = 0;  // V_LDSH: slots of the workgroup's LDS table
    // V_BROW: the accumulator word every row of a group updates -- "this build row has a group" is read off it (its value differs
    // from occ_empty), and the kernel stores no tags -- or -1: tags are stored
    int occ_word = -1;
    uint64_t occ_empty = 0;
    std::vector<int32_t> word_kind;
    std::vector<std::pair<int, int>> agg_words;  // per aggregate: (count word, value word or -1)
    // per aggregate: > 0 for sum / avg over a DECIMAL -- the value is kept as that many limb words from agg_words[k].second on
    // (pa_dec_limb: independent integer sums, put together at output: decimal_host.hpp)
    std::vector<int> agg_limbs;
    std::vector<KeyPart> keys;
    // identity of the state layout (key packing + meaning of every accumulator word): states are only ever merged,
    // folded or emitted under the layout they were accumulated with
    std::string layout_id;
};

// thrown by adopt_layout before anything of the page was launched: the page's signature needs another state layout
struct LayoutChange {};

// jd / bridge: the probe stage between the projections and the aggregation (null: none); the aggregation's channels then index
// the join's output page = [probe output channels, build output channels] (LookupJoinPageBuilder.java:76-139)
Spec make_spec(const pa_filter_project_desc& fp, const pa_hash_aggregation_desc& ag, const pa_lookup_join_desc* jd = nullptr,
               pa_lookup_source* bridge = nullptr);
Spec make_spec(const pa_fused_aggregation_desc* d);
// channels read, short / interned VARCHAR keys: everything of a Spec that follows from its expressions and aggregates
void finalize_spec(Spec& s);
// the staged plan of a Spec (Spec::conjuncts .. n_stages; part of finalize_spec)
void plan_stages(Spec& s);

// Words of a range-table entry, in this order: per used channel its values pointer, its offsets pointer when it is a VARCHAR
// channel, its NULL flags pointer when the layout calls it nullable; then rows | (vec << 32).
int range_entry_words(const Spec& s, const std::vector<ChannelLayout>& layout);
// the translation unit of one tier (`variant`) for pages of one layout signature (fused_codegen.cpp)
KernelInfo generate(const Spec& s, const std::vector<ChannelLayout>& layout, int variant);
// PRESTO_AMD_LDS_PIPE (measurement switch, default 1): 0 = the few-groups tier's head loop over a packed key loads a quad and works on
// it, instead of loading the next quad first.  The switch changes the generated source, hence the kernel's name; an operator's plan
// fingerprint carries it, so that kernels generated under another setting are not shared.
int lds_pipe_level();
// PRESTO_AMD_NT (default 1): the cache policy of the 16-byte column loads of the ungrouped tier's staged page loop.  0 = default-policy
// loads (the source of before the switch, byte for byte), 1 = non-temporal loads for stage 0 (the columns every row reads: each byte
// is read once per pass), 2 = also for the masked loads of the later stages, whose dead quads re-read the column's first line
// (measured slower on Q6: DESIGN section 4).  Part of the plan fingerprint, as PRESTO_AMD_LDS_PIPE is.
int nt_level();

}  // namespace fused
}  // namespace pa
