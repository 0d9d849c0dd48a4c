// op_nested_loop.cpp -- NestedLoopBuildOperator + NestedLoopJoinOperator (cross joins, scalar subqueries, joins over an inequality
// alone) on device, with the FilterAndProject above the join evaluated over the product space.
//
// Reference path replaced:
//   LocalExecutionPlanner.createNestedLoopJoin (…/sql/planner/LocalExecutionPlanner.java: a JoinNode without equi-criteria)
//   NestedLoopBuildOperator (…/operator/join/NestedLoopBuildOperator.java) -> NestedLoopJoinPagesBuilder -> NestedLoopJoinBridge
//   NestedLoopJoinOperator (…/operator/join/NestedLoopJoinOperator.java: NestedLoopOutputIterator, one RLE page per row of the
//     smaller side of every (probe page, build page) pair)
//   the FilterAndProjectOperator directly above it, when the join is given its filter
//
// Contract (include/presto_amd.h): one row per pair (probe row i, build row j) the filter keeps, PROBE-MAJOR -- i ascending, inside
// one i, j ascending -- whatever the page cuts and encodings of either side.  The reference emits the same multiset in another order.
//
// Build: a HeldRows over the build channels some join operator reads.  Probe: a probe page is walked rectangle by rectangle of the
// product -- P probe rows x the whole build, P = max(1, bound / M); one probe row x build ranges when M alone exceeds the bound of an
// output page.  Per rectangle
//   no filter   launch_nested_loop_product: the position lists are arithmetic
//   filter      pa_nl_count_* (survivors per probe row) -> exclusive scan -> ONE read-back (total + error word) -> pa_nl_emit_*
//               (the filter again, (probe_idx, build_pos) written at the row's offset): the product is never materialised
// then PositionGather::copy_positions of the output channels through the two lists.  Every output element has one writer per launch,
// nothing is carried between workgroups, no atomic decides a position: the order is part of the contract.
//
// The pair kernels are generated per (filter, channel layout, lane mapping) around RowCodegen::emit, two lane mappings:
//   variant 0 (pa_nl_*_rows)   lanes over probe rows: a lane keeps its probe row's filter channels in registers and loops over the build
//                              rows, whose filter channels come through LDS in chunks of kNestedLoopLdsChunk rows (all lanes read
//                              build row jj at one address: a broadcast); a lane's survivors are one contiguous run of the output
//   variant 1 (pa_nl_*_build)  lanes over build rows: a wave owns one probe row (its values are wave-uniform), its lanes take 64
//                              consecutive build rows per step, __ballot + popcount of the lanes below rank the survivors of a step;
//                              build-column loads and position stores are coalesced
#include <atomic>
#include <map>
#include <mutex>
#include <sstream>

#include "exprgen.hpp"
#include "held_rows.hpp"
#include "jit.hpp"
#define PA_ARGS_STDINT
#include "kernels/pa_args.h"
#include "keyed_operator.hpp"
#include "nested_loop_kernels.hpp"
#include "rowgen.hpp"

namespace pa {

// NestedLoopJoinBridge / NestedLoopJoinPages: what the builder publishes and the join operators read
struct NestedLoopPagesImpl {
    std::mutex mu;                         // guards everything up to `frozen`
    bool has_builder = false;
    std::vector<int32_t> types;            // the build page's types, once a builder exists
    std::vector<bool> read;                // build channels some join operator reads
    bool frozen = false;                   // the builder has taken its first page with rows: `read` is what it holds
    HeldRows rows;                         // written by the builder alone until `built`
    std::atomic<int32_t> error{0};         // the build failed (a pa_status): published with `built`, the joins raise it
    std::atomic<bool> built{false};        // set last
};

}  // namespace pa

struct pa_nested_loop_pages {
    std::shared_ptr<pa::NestedLoopPagesImpl> impl;
};

namespace pa {
namespace {

// Which lane mapping a rectangle of n probe rows x m build rows takes (measured: DESIGN.md section 4, NESTED LOOP JOIN;
// profiles/nested_loop_bench.json).  Variant 0 puts one probe row on a lane, so a rectangle gives it n / 256 workgroups: from four per
// CU on (2^18 rows) it was the faster one at every build size (0.47-0.70 of variant 1's time), at 2^16 rows and below variant 1 was
// (1.07-4.9 x faster at 256 build rows and more; one exception, the band filter at 2^16 rows, 0.76).  Below 64 build rows a wave of
// variant 1 has idle lanes in its only step, and variant 0 was never behind (16 build rows: 0.70-1.01 of variant 1's time).
constexpr int64_t kNestedLoopRowsForVariant0 = (int64_t)1 << 18;
constexpr int64_t kNestedLoopBuildRowsForVariant1 = 64;

bool known_type(int32_t t) { return t >= PA_BIGINT && t <= PA_LONG_DECIMAL; }

// the filter of a join over a pair: channels [0, nb) the build page's, [nb, nb + np) the probe page's
struct NlPlan {
    int nb = 0, np = 0;
    std::vector<int32_t> types;   // of the pair's channels
    OwnedExpr filter;
    std::vector<bool> used;       // channels the filter reads
};

NlPlan make_plan(const std::vector<int32_t>& build_types, const std::vector<int32_t>& probe_types, const pa_expr& f)
{
    NlPlan p;
    p.nb = (int)build_types.size();
    p.np = (int)probe_types.size();
    p.types = build_types;
    p.types.insert(p.types.end(), probe_types.begin(), probe_types.end());
    p.filter = OwnedExpr::copy(f);
    PA_REQUIRE(p.filter.root_type() == PA_BOOLEAN, PA_ERR_INVALID_ARGUMENT, "filter must be BOOLEAN");
    std::set<int32_t> used;
    p.filter.collect_channels(&used);
    p.used.assign(p.types.size(), false);
    for (int32_t c : used) {
        PA_REQUIRE(c >= 0 && c < p.nb + p.np, PA_ERR_INVALID_ARGUMENT, "filter references a channel outside the build and probe pages");
        p.used[c] = true;
    }
    return p;
}

// the arguments of the row function for channel c read at `idx` of the arrays V / O / NL (the order of row_params)
std::string channel_args(const ChannelLayout& l, const std::string& V, const std::string& O, const std::string& NL, const std::string& idx)
{
    std::string a;
    switch (l.type) {
        case PA_BIGINT:
        case PA_DECIMAL: a = ", ((const i64*)" + V + ")[" + idx + "]"; break;
        case PA_LONG_DECIMAL: a = ", pa_ld_read((const u64*)" + V + " + 2 * (" + idx + "))"; break;
        case PA_DOUBLE: a = ", ((const double*)" + V + ")[" + idx + "]"; break;
        case PA_INTEGER:
        case PA_DATE: a = ", (i64)((const i32*)" + V + ")[" + idx + "]"; break;
        case PA_REAL: a = ", ((const float*)" + V + ")[" + idx + "]"; break;
        case PA_BOOLEAN: a = ", ((const u8*)" + V + ")[" + idx + "] != 0"; break;
        case PA_VARCHAR: a = ", (const u8*)" + V + " + " + O + "[" + idx + "], " + O + "[(" + idx + ") + 1] - " + O + "[" + idx + "]"; break;
        default: throw Error(PA_ERR_NOT_SUPPORTED, "column type not supported on device");
    }
    if (l.nullable) a += ", " + NL + "[" + idx + "] != 0";
    return a;
}

// LDS bytes per build row of the build channels the filter reads (a VARCHAR: its offset; the bytes stay in memory)
int staged_row_bytes(const NlPlan& p, const std::vector<ChannelLayout>& layout)
{
    int bytes = 0;
    for (int c = 0; c < p.nb; c++) {
        if (!p.used[c]) continue;
        bytes += (layout[c].type == PA_VARCHAR ? 4 : type_width(layout[c].type)) + (layout[c].nullable ? 1 : 0);
    }
    return bytes;
}

// One translation unit per (plan, layout, variant): the predicate, its count form and its emit form
std::string generate_nl(const NlPlan& p, const std::vector<ChannelLayout>& layout, int variant)
{
    RowInputs ri;
    ri.n_in = p.nb + p.np;
    ri.used = p.used;
    ri.short_bound.assign(ri.n_in, 0);
    std::ostringstream src;
    // the predicate over one pair: TRUE keeps it, NULL counts as false (PageFunctionCompiler.java:539-542)
    src << "__device__ __forceinline__ bool pa_nl_keep(const PaNlArgs& a" << row_params(ri, layout) << ")\n{\n";
    {
        RowCodegen gen(layout, "a.err");
        std::ostringstream body;
        GenValue f = gen.emit(p.filter, body);
        src << body.str() << "return " << (f.nullable() ? "(!" + f.n + " && " + f.v + ")" : f.v) << ";\n}\n\n";
    }
    const ColumnNames nm;
    // the probe row's channels, loaded once per lane (variant 0) / per wave (variant 1) into locals
    std::ostringstream probe_decl;
    std::string probe_args;
    {
        RowInputs pr = ri;
        for (int c = 0; c < p.nb; c++) pr.used[c] = false;
        probe_args = scalar_loads(pr, layout, "pa_i", "p", probe_decl, nm);
    }
    const int row_bytes = staged_row_bytes(p, layout);
    const bool staged = variant == 0 && row_bytes > 0 && row_bytes * kNestedLoopLdsChunk + 64 <= kNestedLoopLdsBytes;
    auto build_args = [&](const std::string& global_idx, const std::string& lds_idx) {
        std::string a;
        for (int c = 0; c < p.nb; c++) {
            if (!p.used[c]) continue;
            const std::string C = std::to_string(c);
            if (staged) a += channel_args(layout[c], layout[c].type == PA_VARCHAR ? nm.v(c) : "pa_sv" + C, "pa_so" + C, "pa_sn" + C, lds_idx);
            else a += channel_args(layout[c], nm.v(c), nm.o(c), nm.nl(c), global_idx);
        }
        return a;
    };
    const std::string CH = std::to_string(kNestedLoopLdsChunk);
    for (int emit = 0; emit < 2; emit++) {
        if (variant == 0) {
            src << "extern \"C\" __global__ __launch_bounds__(256) void PA_K(" << (emit ? "pa_nl_emit_rows" : "pa_nl_count_rows") << ")(PaNlArgs a)\n{\n";
            if (staged) {
                for (int c = 0; c < p.nb; c++) {
                    if (!p.used[c]) continue;
                    const std::string C = std::to_string(c);
                    switch (layout[c].type == PA_VARCHAR ? 0 : type_width(layout[c].type)) {
                        case 0: src << "    __shared__ __attribute__((aligned(16))) i32 pa_so" << C << "[" << CH << " + 1];\n"; break;
                        case 16: src << "    __shared__ __attribute__((aligned(16))) u64 pa_sv" << C << "[2 * " << CH << "];\n"; break;
                        case 8: src << "    __shared__ __attribute__((aligned(16))) u64 pa_sv" << C << "[" << CH << "];\n"; break;
                        case 4: src << "    __shared__ __attribute__((aligned(16))) u32 pa_sv" << C << "[" << CH << "];\n"; break;
                        default: src << "    __shared__ __attribute__((aligned(16))) u8 pa_sv" << C << "[" << CH << "];\n"; break;
                    }
                    if (layout[c].nullable) src << "    __shared__ __attribute__((aligned(16))) u8 pa_sn" << C << "[" << CH << "];\n";
                }
            }
            // (a lane past the rectangle's rows still takes part in the staging and its barriers)
            src << "    const i32 pa_r = (i32)(blockIdx.x * 256u + threadIdx.x);\n    const bool pa_live = pa_r < a.n;\n"
                   "    const i64 pa_i = (i64)a.i0 + (pa_live ? pa_r : 0);\n    "
                << probe_decl.str() << "\n";
            src << (emit ? "    i32 pa_at = pa_live ? a.offsets[pa_r] : 0;\n" : "    i32 pa_cnt = 0;\n");
            src << "    for (i32 pa_c0 = 0; pa_c0 < a.m; pa_c0 += " << CH << ") {\n        const i32 pa_cn = a.m - pa_c0 < " << CH << " ? a.m - pa_c0 : " << CH << ";\n";
            if (staged) {
                src << "        __syncthreads();\n        for (i32 pa_t = (i32)threadIdx.x; pa_t <= pa_cn; pa_t += 256) {\n            const i32 pa_g = a.j0 + pa_c0 + pa_t;\n";
                for (int c = 0; c < p.nb; c++) {
                    if (!p.used[c]) continue;
                    const std::string C = std::to_string(c);
                    if (layout[c].type == PA_VARCHAR) src << "            pa_so" << C << "[pa_t] = " << nm.o(c) << "[pa_g];\n";
                }
                src << "            if (pa_t < pa_cn) {\n";
                for (int c = 0; c < p.nb; c++) {
                    if (!p.used[c]) continue;
                    const std::string C = std::to_string(c);
                    switch (layout[c].type == PA_VARCHAR ? 0 : type_width(layout[c].type)) {
                        case 0: break;
                        case 16:
                            src << "                pa_sv" << C << "[2 * pa_t] = ((const u64*)" << nm.v(c) << ")[2 * (i64)pa_g]; pa_sv" << C << "[2 * pa_t + 1] = ((const u64*)" << nm.v(c)
                                << ")[2 * (i64)pa_g + 1];\n";
                            break;
                        case 8: src << "                pa_sv" << C << "[pa_t] = ((const u64*)" << nm.v(c) << ")[pa_g];\n"; break;
                        case 4: src << "                pa_sv" << C << "[pa_t] = ((const u32*)" << nm.v(c) << ")[pa_g];\n"; break;
                        default: src << "                pa_sv" << C << "[pa_t] = ((const u8*)" << nm.v(c) << ")[pa_g];\n"; break;
                    }
                    if (layout[c].nullable) src << "                pa_sn" << C << "[pa_t] = " << nm.nl(c) << "[pa_g];\n";
                }
                src << "            }\n        }\n        __syncthreads();\n";
            }
            src << "        if (pa_live) {\n            for (i32 pa_jj = 0; pa_jj < pa_cn; pa_jj++) {\n                const i64 pa_j = (i64)a.j0 + pa_c0 + pa_jj;\n"
                << "                if (pa_nl_keep(a" << build_args("pa_j", "pa_jj") << probe_args << ")) {\n";
            if (emit) src << "                    a.probe_idx[pa_at] = (i32)pa_i;\n                    a.build_pos[pa_at] = (i32)pa_j;\n                    pa_at++;\n";
            else src << "                    pa_cnt++;\n";
            src << "                }\n            }\n        }\n    }\n";
            if (!emit) src << "    if (pa_live) a.counts[pa_r] = pa_cnt;\n";
            src << "}\n\n";
        }
        else {
            src << "extern \"C\" __global__ __launch_bounds__(256) void PA_K(" << (emit ? "pa_nl_emit_build" : "pa_nl_count_build") << ")(PaNlArgs a)\n{\n";
            src << "    const i32 pa_lane = (i32)(threadIdx.x & 63u);\n"
                   "    const i32 pa_r = __builtin_amdgcn_readfirstlane((i32)(blockIdx.x * 4u + (threadIdx.x >> 6)));\n"
                   "    if (pa_r >= a.n) return;\n    const i64 pa_i = (i64)a.i0 + pa_r;\n    "
                << probe_decl.str() << "\n";
            src << (emit ? "    i32 pa_at = a.offsets[pa_r];\n" : "    i32 pa_cnt = 0;\n");
            src << "    for (i32 pa_c0 = 0; pa_c0 < a.m; pa_c0 += 64) {\n        const i32 pa_jj = pa_c0 + pa_lane;\n        const i64 pa_j = (i64)a.j0 + pa_jj;\n        bool pa_k = false;\n"
                << "        if (pa_jj < a.m) pa_k = pa_nl_keep(a" << build_args("pa_j", "pa_j") << probe_args << ");\n"
                << "        const u64 pa_mask = __ballot(pa_k);\n";
            if (emit) {
                src << "        if (pa_k) {\n            const i32 pa_p = pa_at + (i32)__popcll(pa_mask & ((1ULL << pa_lane) - 1ULL));\n"
                       "            a.probe_idx[pa_p] = (i32)pa_i;\n            a.build_pos[pa_p] = (i32)pa_j;\n        }\n        pa_at += (i32)__popcll(pa_mask);\n";
            }
            else src << "        pa_cnt += (i32)__popcll(pa_mask);\n";
            src << "    }\n";
            if (!emit) src << "    if (pa_lane == 0) a.counts[pa_r] = pa_cnt;\n";
            src << "}\n\n";
        }
    }
    return src.str();
}

// ---- descriptor checks (before the device is asked for; an invalid argument before a refusal) -------------------------------------------
void check_types_known(const int32_t* types, int32_t count, const char* what)
{
    for (int32_t c = 0; c < count; c++) PA_REQUIRE(known_type(types[c]) || types[c] == PA_ROW, PA_ERR_INVALID_ARGUMENT, std::string("unknown ") + what + " channel type");
}
void check_types_carried(const std::vector<int32_t>& types, const char* what)
{
    for (int32_t t : types) check_carried_type(t, what);
}

void* checked_stream(const pa_nested_loop_build_desc* d)
{
    PA_REQUIRE(d != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    PA_REQUIRE(d->input_channel_count >= 0, PA_ERR_INVALID_ARGUMENT, "negative build channel count");
    PA_REQUIRE(d->input_channel_count == 0 || d->input_types != nullptr, PA_ERR_INVALID_ARGUMENT, "build types are null");
    check_types_known(d->input_types, d->input_channel_count, "build");
    PA_REQUIRE(d->input_channel_count <= PA_NL_MAX_CHANNELS, PA_ERR_NOT_SUPPORTED, "at most 64 build channels");
    for (int32_t c = 0; c < d->input_channel_count; c++) check_carried_type(d->input_types[c], "build");
    return d->stream;
}

class NestedLoopBuildOperator : public pa_operator {
public:
    NestedLoopBuildOperator(const pa_nested_loop_build_desc* d, pa_nested_loop_pages* pages) : stream_(checked_stream(d))
    {
        PA_REQUIRE(pages != nullptr && pages->impl != nullptr, PA_ERR_INVALID_ARGUMENT, "pages handle is null");
        std::lock_guard<std::mutex> lock(pages->impl->mu);
        PA_REQUIRE(!pages->impl->has_builder, PA_ERR_ILLEGAL_STATE, "the handle already has a builder");
        pages_ = pages->impl;
        pages_->types.assign(d->input_types, d->input_types + d->input_channel_count);
        pages_->read.assign(pages_->types.size(), false);
        pages_->has_builder = true;
    }
    ~NestedLoopBuildOperator() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t main_stream() override { return stream_.get(); }

    bool needs_input() override { return !finishing_; }

    // NestedLoopBuildOperator.addInput -> NestedLoopJoinPagesBuilder.addPage
    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(!finishing_, PA_ERR_ILLEGAL_STATE, "Operator is already finishing");
        NestedLoopPagesImpl& p = *pages_;
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)p.types.size(), PA_ERR_INVALID_ARGUMENT, "page does not match the build types");
        const int32_t m = page->position_count;
        if (m <= 0) return;
        if (!held_) {
            // the channels held are decided with the first rows: what the join operators created so far read, everything when there is none
            std::lock_guard<std::mutex> lock(p.mu);
            bool any = false;
            for (bool r : p.read) any = any || r;
            if (!any) p.read.assign(p.types.size(), true);
            p.rows.init(p.types, p.read);
            p.frozen = true;
            held_ = true;
        }
        PA_REQUIRE(p.rows.rows + m <= INT32_MAX, PA_ERR_INSUFFICIENT_RESOURCES, "build side exceeds 2^31 positions");
        hipStream_t s = stream_.get();
        try {
            DevPage dp = stager_.stage(page, &p.rows.held, s);   // (dictionary and RLE blocks come out flat)
            p.rows.append_page(dp, m, s);
            // (the stager's arena is overwritten by the next page; a device page is the caller's again when the call returns)
            PA_HIP(hipStreamSynchronize(s));
        }
        catch (const Error& e) {
            fail(e.code);
            throw;
        }
    }

    // finish: the rows are published (NestedLoopJoinPagesBuilder.build -> NestedLoopJoinBridge.setPages)
    void finish() override
    {
        if (finishing_) return;
        finishing_ = true;
        (void)hipStreamSynchronize(stream_.get());
        pages_->built.store(true);
    }
    bool get_output(pa_page*) override { return false; }
    bool is_finished() override { return finishing_; }
    int64_t memory_bytes() override { return (int64_t)pages_->rows.bytes(); }

private:
    // (as HashBuilderOperator: the error is published with `built`, the joins raise it instead of waiting)
    void fail(int32_t code)
    {
        finishing_ = true;
        pages_->error.store(code);
        pages_->built.store(true);
    }

    Stream stream_;
    PageStager stager_;
    std::shared_ptr<NestedLoopPagesImpl> pages_;
    bool held_ = false, finishing_ = false;
};

// what of a join descriptor can be checked without the handle
void* checked_stream(const pa_nested_loop_join_desc* d)
{
    PA_REQUIRE(d != nullptr, PA_ERR_INVALID_ARGUMENT, "descriptor is null");
    PA_REQUIRE(d->probe_channel_count >= 0 && d->probe_output_channel_count >= 0 && d->build_output_channel_count >= 0, PA_ERR_INVALID_ARGUMENT, "negative channel count");
    PA_REQUIRE(d->probe_channel_count == 0 || d->probe_types != nullptr, PA_ERR_INVALID_ARGUMENT, "probe types are null");
    PA_REQUIRE(d->probe_output_channel_count == 0 || d->probe_output_channels != nullptr, PA_ERR_INVALID_ARGUMENT, "probe output channels are null");
    PA_REQUIRE(d->build_output_channel_count == 0 || d->build_output_channels != nullptr, PA_ERR_INVALID_ARGUMENT, "build output channels are null");
    check_channels(d->probe_output_channels, d->probe_output_channel_count, d->probe_channel_count, "probe output");
    check_output_mem(d->output_mem);
    check_types_known(d->probe_types, d->probe_channel_count, "probe");
    return d->stream;
}

// ... and with the build types: the rest of the invalid arguments, then the refusals.  Returns the filter's plan (empty without one)
NlPlan check_join(const pa_nested_loop_join_desc* d, const std::vector<int32_t>& build_types)
{
    check_channels(d->build_output_channels, d->build_output_channel_count, (int32_t)build_types.size(), "build output");
    const std::vector<int32_t> probe_types(d->probe_types, d->probe_types + d->probe_channel_count);
    NlPlan plan;
    if (d->filter) plan = make_plan(build_types, probe_types, *d->filter);
    check_types_carried(probe_types, "probe");
    check_types_carried(build_types, "build");
    PA_REQUIRE(d->probe_output_channel_count + d->build_output_channel_count > 0, PA_ERR_NOT_SUPPORTED, "a nested-loop join without output channels is not on the device path");
    PA_REQUIRE((int64_t)probe_types.size() + (int64_t)build_types.size() <= PA_NL_MAX_CHANNELS, PA_ERR_NOT_SUPPORTED, "at most 64 channels on both sides together");
    if (d->filter) {
        // an expression the generator does not take is refused here, not at the first page: no refusal depends on the layout signature
        std::vector<ChannelLayout> dry(plan.types.size());
        for (size_t c = 0; c < dry.size(); c++) dry[c].type = plan.types[c];
        (void)generate_nl(plan, dry, 0);
    }
    return plan;
}

int64_t max_output_rows()
{
    const char* e = getenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS");  // (as op_join.cpp: tests exercise the cutting with a small bound)
    const int64_t cap = (int64_t)1 << 30;
    return e ? std::min(std::max<int64_t>(strtoll(e, nullptr, 10), 1), cap) : cap;
}

class NestedLoopJoinOperator : public pa_operator {
public:
    NestedLoopJoinOperator(const pa_nested_loop_join_desc* d, pa_nested_loop_pages* pages) : pages_(claim(d, pages)), stream_(d->stream)
    {
        probe_types_.assign(d->probe_types, d->probe_types + d->probe_channel_count);
        probe_out_.assign(d->probe_output_channels, d->probe_output_channels + d->probe_output_channel_count);
        build_out_.assign(d->build_output_channels, d->build_output_channels + d->build_output_channel_count);
        output_mem_ = d->output_mem;
        needed_.assign(probe_types_.size(), false);
        for (int32_t c : probe_out_) needed_[c] = true;
        for (int c = 0; c < plan_.np; c++) needed_[c] = needed_[c] || plan_.used[plan_.nb + c];
        kept_.init(probe_types_, needed_);
        const char* e = getenv("PRESTO_AMD_NL_VARIANT");
        if (e && (e[0] == '0' || e[0] == '1') && e[1] == 0) forced_variant_ = e[0] - '0';
        ctl_ = static_cast<int32_t*>(ctl_buf_.ensure(64));  // [0] err [1] the rectangle's surviving pairs
        PA_HIP(hipMemsetAsync(ctl_, 0, 64, stream_.get()));
        out_cols_.resize(probe_out_.size() + build_out_.size());
    }
    ~NestedLoopJoinOperator() override { (void)hipStreamSynchronize(stream_.get()); }
    hipStream_t private_stream() override { return stream_.owned() ? stream_.get() : nullptr; }
    hipStream_t main_stream() override { return stream_.get(); }

    bool needs_input() override { return !finishing_ && !pending_ && pages_->built.load(); }
    bool is_blocked() override { return !pages_->built.load(); }

    void add_input(const pa_page* page) override
    {
        PA_REQUIRE(pages_->built.load(), PA_ERR_ILLEGAL_STATE, "the build rows are not published yet");
        if (int32_t e = pages_->error.load()) throw Error(e, "the nested-loop build failed on device");
        PA_REQUIRE(!finishing_ && !pending_, PA_ERR_ILLEGAL_STATE, "Operator does not need input");
        PA_REQUIRE(page != nullptr && page->channel_count == (int32_t)probe_types_.size(), PA_ERR_INVALID_ARGUMENT, "probe page does not match the probe types");
        const int64_t m = pages_->rows.rows;
        if (page->position_count <= 0 || m == 0) return;
        hipStream_t s = stream_.get();
        in_ = stager_.stage(page, &needed_, s);
        for (size_t c = 0; c < needed_.size(); c++) {
            PA_REQUIRE(!needed_[c] || in_.cols[c].type == probe_types_[c], PA_ERR_INVALID_ARGUMENT, "page block type does not match the declared probe type");
        }
        // A page that comes out as several: the operator upstream may be given its next page in between, and a device page some operator
        // returned is that operator's again with its next call -- the channels still to be read are kept (as the lookup join keeps them)
        const int64_t bound = max_output_rows();
        const bool several = m > bound || (int64_t)in_.n > std::max<int64_t>(1, bound / m);
        if (several && page->mem == PA_MEM_DEVICE && (page->flags & PA_PAGE_STABLE) == 0) {
            kept_.reset();
            kept_.append_page(in_, in_.n, s);
            for (size_t c = 0; c < needed_.size(); c++) {
                if (needed_[c]) in_.cols[c] = kept_.view((int32_t)c);
            }
            PA_HIP(hipStreamSynchronize(s));
        }
        next_i_ = 0;
        next_j_ = 0;
        pending_ = true;
    }

    bool get_output(pa_page* out) override
    {
        while (pending_) {
            // the next rectangle of the product, probe-major
            const int64_t m_all = pages_->rows.rows, bound = max_output_rows();
            int32_t i0 = next_i_, n = 1, j0 = 0, m = (int32_t)m_all;
            if (m_all <= bound) {
                n = (int32_t)std::min<int64_t>(std::max<int64_t>(1, bound / m_all), in_.n - i0);
                next_i_ += n;
            }
            else {
                j0 = next_j_;
                m = (int32_t)std::min<int64_t>(bound, m_all - j0);
                next_j_ += m;
                if (next_j_ == m_all) {
                    next_j_ = 0;
                    next_i_++;
                }
            }
            pending_ = next_i_ < in_.n;
            int32_t total = 0;
            try {
                total = pair_positions(i0, n, j0, m);
                if (total > 0) gather_output(total, out);
            }
            catch (...) {
                pending_ = false;   // nothing of this rectangle, nor of the rest of the page, is emitted
                throw;
            }
            if (total > 0) return true;
        }
        return false;
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finishing_ && !pending_; }
    int64_t memory_bytes() override
    {
        return (int64_t)(stager_.bytes() + kept_.bytes() + probe_idx_.capacity() + build_pos_.capacity() + counts_.capacity() + scan_temp_.capacity() + gather_.bytes());
    }

private:
    // the descriptor checks, all of them before the device is asked for; fills plan_ and registers the build channels read
    std::shared_ptr<NestedLoopPagesImpl> claim(const pa_nested_loop_join_desc* d, pa_nested_loop_pages* pages)
    {
        (void)checked_stream(d);
        PA_REQUIRE(pages != nullptr && pages->impl != nullptr, PA_ERR_INVALID_ARGUMENT, "pages handle is null");
        NestedLoopPagesImpl& p = *pages->impl;
        std::lock_guard<std::mutex> lock(p.mu);
        PA_REQUIRE(p.has_builder, PA_ERR_ILLEGAL_STATE, "the handle has no builder yet: the join needs the build types");
        plan_ = check_join(d, p.types);
        require_device();
        std::vector<bool> reads(p.types.size(), false);
        for (int32_t i = 0; i < d->build_output_channel_count; i++) reads[d->build_output_channels[i]] = true;
        for (int c = 0; c < plan_.nb; c++) reads[c] = reads[c] || plan_.used[c];
        for (size_t c = 0; c < reads.size(); c++) {
            PA_REQUIRE(!reads[c] || !p.frozen || p.read[c], PA_ERR_ILLEGAL_STATE, "the builder has taken rows already and does not hold a build channel this join reads");
            if (reads[c]) p.read[c] = true;
        }
        return pages->impl;
    }

    struct Compiled {
        hipFunction_t count_fn = nullptr, emit_fn = nullptr;
        std::string name;
    };
    // (the code object is jit.hpp's to cache, under the key of its source: the filter, the layout signature and the variant)
    const Compiled& kernel_for(int variant, const std::string& sig, const std::vector<ChannelLayout>& layout)
    {
        const std::string key = std::to_string(variant) + sig;
        auto it = compiled_.find(key);
        if (it != compiled_.end()) return it->second;
        const std::string source = generate_nl(plan_, layout, variant);
        Compiled c;
        JitKernel k = jit_get(source, variant == 0 ? "pa_nl_count_rows" : "pa_nl_count_build");
        c.count_fn = k.fn;
        c.name = k.name;
        c.emit_fn = jit_get(source, variant == 0 ? "pa_nl_emit_rows" : "pa_nl_emit_build").fn;
        return compiled_[key] = c;
    }

    // (probe_idx, build_pos) of the rectangle's surviving pairs into probe_idx_ / build_pos_; returns their count
    int32_t pair_positions(int32_t i0, int32_t n, int32_t j0, int32_t m)
    {
        hipStream_t s = stream_.get();
        if (!plan_.filter.nodes.size()) {
            const int64_t total = (int64_t)n * m;
            launch_nested_loop_product(i0, n, j0, m, static_cast<int32_t*>(probe_idx_.ensure((size_t)total * 4)), static_cast<int32_t*>(build_pos_.ensure((size_t)total * 4)), s);
            return (int32_t)total;
        }
        const HeldRows& build = pages_->rows;
        PaNlArgs a;
        memset(&a, 0, sizeof a);
        std::vector<ChannelLayout> layout(plan_.types.size());
        std::string sig;
        for (size_t c = 0; c < layout.size(); c++) {
            layout[c].type = plan_.types[c];
            if (plan_.used[c]) {
                const DevColumn col = (int)c < plan_.nb ? build.view((int32_t)c) : in_.cols[c - plan_.nb];
                a.v[c] = col.values;
                a.o[c] = col.offsets;
                a.nl[c] = col.nulls;
                layout[c].nullable = col.nulls != nullptr;
            }
            sig += layout[c].nullable ? 'n' : '-';
        }
        const int variant = forced_variant_ >= 0 ? forced_variant_ : (n >= kNestedLoopRowsForVariant0 || m < kNestedLoopBuildRowsForVariant1 ? 0 : 1);
        const Compiled& ck = kernel_for(variant, sig, layout);
        a.i0 = i0;
        a.n = n;
        a.j0 = j0;
        a.m = m;
        a.counts = static_cast<int32_t*>(counts_.ensure((size_t)n * 4));
        a.offsets = a.counts;   // scanned in place
        a.err = ctl_;
        const unsigned grid = variant == 0 ? (unsigned)(((int64_t)n + 255) / 256) : (unsigned)(((int64_t)n + 3) / 4);
        void* params[] = {&a};
        timer.set_name(ck.name);
        timer.begin(s);
        PA_HIP(hipModuleLaunchKernel(ck.count_fn, grid, 1, 1, 256, 1, 1, 0, s, params, nullptr));
        timer.end(s);
        launch_exclusive_scan_i32(a.counts, a.counts, n, ctl_ + 1, scan_temp_.ensure(scan_temp_bytes(n)), s);
        int32_t h[2] = {0, 0};
        read_back(h, ctl_, 8, s);   // the one round trip of a rectangle besides the gathers' per VARCHAR output channel
        if (h[0] != 0) {
            PA_HIP(hipMemsetAsync(ctl_, 0, 4, s));
            switch (h[0]) {   // (the statuses and words of FilterAndProject)
                case PA_ERR_NUMERIC_VALUE_OUT_OF_RANGE: throw Error(h[0], "numeric value out of range (bigint/integer arithmetic overflow)");
                case PA_ERR_DIVISION_BY_ZERO: throw Error(h[0], "Division by zero");
                default: throw Error(h[0], "device-side error");
            }
        }
        const int32_t total = h[1];
        PA_REQUIRE(total >= 0 && (int64_t)total <= (int64_t)n * m, PA_ERR_DEVICE, "nested-loop join: surviving pairs out of range");
        if (total == 0) return 0;
        a.probe_idx = static_cast<int32_t*>(probe_idx_.ensure((size_t)total * 4));
        a.build_pos = static_cast<int32_t*>(build_pos_.ensure((size_t)total * 4));
        PA_HIP(hipModuleLaunchKernel(ck.emit_fn, grid, 1, 1, 256, 1, 1, 0, s, params, nullptr));
        return total;
    }

    // Block.copyPositions of the output channels: the probe's by probe_idx_ out of the staged page, the build's by build_pos_ out of the
    // held rows
    void gather_output(int32_t total, pa_page* out)
    {
        hipStream_t s = stream_.get();
        size_t oc = 0;
        for (int32_t c : probe_out_) gather_column(in_.cols[c], probe_idx_.as<int32_t>(), total, out_cols_[oc++], s);
        for (int32_t c : build_out_) gather_column(pages_->rows.view(c), build_pos_.as<int32_t>(), total, out_cols_[oc++], s);
        publish_output(out_cols_, total, output_mem_, s, out, out_storage_);
    }
    void gather_column(const DevColumn& src, const int32_t* positions, int32_t count, OutColumn& o, hipStream_t s)
    {
        if (!src.varwidth) {
            gather_.copy_positions(src, positions, count, o, s);
            return;
        }
        // (the output rows of a product multiply: the byte total is checked in 64 bits, as the lookup join's)
        o.type = src.type;
        o.varwidth = true;
        o.has_nulls = src.nulls != nullptr;
        o.is_view = false;
        o.host_ready = false;
        if (src.nulls) launch_gather_nulls(src.nulls, positions, count, static_cast<uint8_t*>(o.nulls.ensure((size_t)count)), s);
        gather_.copy_varwidth(src, positions, count, o.offsets, o.values, s, "a join output page holds more than 2 GiB of VARCHAR bytes");
    }

    NlPlan plan_;   // (filled by claim(), before the members below are constructed)
    std::shared_ptr<NestedLoopPagesImpl> pages_;
    Stream stream_;
    PageStager stager_;
    std::vector<int32_t> probe_types_, probe_out_, build_out_;
    std::vector<bool> needed_;
    int32_t output_mem_ = PA_MEM_HOST;
    int forced_variant_ = -1;
    DevPage in_;
    HeldRows kept_;   // the probe page's channels, when the page outlives the call that brought it
    int32_t next_i_ = 0;   // first probe row whose pairs are still to come
    int64_t next_j_ = 0;   // ... and its first build row (only when one probe row's pairs exceed the bound)
    bool pending_ = false, finishing_ = false;
    std::map<std::string, Compiled> compiled_;
    DevBuf ctl_buf_, counts_, scan_temp_, probe_idx_, build_pos_;
    int32_t* ctl_ = nullptr;
    PositionGather gather_;
    std::vector<OutColumn> out_cols_;
    std::vector<pa_column> out_storage_;
};

}  // namespace

pa_nested_loop_pages* nested_loop_pages_new()
{
    pa_nested_loop_pages* p = new pa_nested_loop_pages;
    p->impl = std::make_shared<NestedLoopPagesImpl>();
    return p;
}
void nested_loop_pages_delete(pa_nested_loop_pages* pages) { delete pages; }

int64_t nested_loop_pages_rows(pa_nested_loop_pages* pages)
{
    PA_REQUIRE(pages != nullptr && pages->impl != nullptr, PA_ERR_INVALID_ARGUMENT, "pages handle is null");
    PA_REQUIRE(pages->impl->built.load(), PA_ERR_ILLEGAL_STATE, "the build rows are not published yet");
    return pages->impl->rows.rows;
}

pa_operator* make_nested_loop_build(const pa_nested_loop_build_desc* desc, pa_nested_loop_pages* pages) { return new NestedLoopBuildOperator(desc, pages); }
pa_operator* make_nested_loop_join(const pa_nested_loop_join_desc* desc, pa_nested_loop_pages* pages) { return new NestedLoopJoinOperator(desc, pages); }

// the pair kernels of a plan without a device.  variant bit 0: the lane mapping; bit 1: the channels the filter reads carry NULL flags
std::string nested_loop_source_for_desc(const pa_nested_loop_join_desc* desc, const pa_nested_loop_build_desc* build, int variant)
{
    (void)checked_stream(build);
    (void)checked_stream(desc);
    PA_REQUIRE(variant >= 0 && variant <= 3, PA_ERR_INVALID_ARGUMENT, "unknown nested-loop kernel variant");
    PA_REQUIRE(desc->filter != nullptr, PA_ERR_INVALID_ARGUMENT, "a nested-loop join without a filter has no generated kernel");
    const NlPlan plan = check_join(desc, std::vector<int32_t>(build->input_types, build->input_types + build->input_channel_count));
    std::vector<ChannelLayout> layout(plan.types.size());
    for (size_t c = 0; c < layout.size(); c++) {
        layout[c].type = plan.types[c];
        layout[c].nullable = (variant & 2) != 0 && plan.used[c];
    }
    return generate_nl(plan, layout, variant & 1);
}

}  // namespace pa
