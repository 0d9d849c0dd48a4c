// op_fused_kernels.cpp -- FusedAggregationOperator (op_fused.hpp): the code a launch runs.  One Compiled per (plan, layout signature,
// variant, device), shared by the operators of the process (kernel_for), the state layout an operator adopts from its first kernel,
// and the choice between the plain and the staged kernel of the ungrouped tier (staged_kernel before, staged_decide after a launch).
#include <cmath>

#include "op_fused.hpp"

namespace pa {
namespace fused_op {

int FusedAggregationOperator::staged_mode()
{
    const char* e = getenv("PRESTO_AMD_STAGED");
    if (!e || !strcmp(e, "auto")) return 2;
    return atoi(e) != 0 ? 1 : 0;
}

// the staged kernel for rows of this page, or null: the plain one
const FusedAggregationOperator::Compiled* FusedAggregationOperator::staged_kernel(const std::string& sig, const std::vector<ChannelLayout>& layout, int64_t rows)
{
    const int m = staged_mode();
    if (m == 0 || spec_.n_stages < 2 || staged_refused_ || (m == 2 && rows < kStagedMinRows)) return nullptr;
    const Compiled* ck = nullptr;
    try {
        ck = &kernel_for(sig, layout, V_GLOBAL_S);
    }
    catch (const Error& e) {
        if (e.code != PA_ERR_NOT_SUPPORTED) throw;
        staged_refused_ = true;  // (column types the staged loop does not load)
        return nullptr;
    }
    return m == 2 && ck->staged_verdict.load(std::memory_order_relaxed) == 2 ? nullptr : ck;
}

// Bytes per row the staged loads are expected to move, from the rows alive in front of every stage, for independent rows in
// 128-byte lines: a line of stage k is fetched when one of its 128 / w_k rows is alive.
double FusedAggregationOperator::staged_bytes(const std::vector<int>& w, const std::vector<double>& alive)
{
    double b = 0;
    for (size_t k = 0; k < w.size(); k++) {
        if (w[k] <= 0) continue;
        const double p = k == 0 ? 1.0 : alive[k - 1];
        b += w[k] * (1.0 - std::pow(1.0 - p, 128.0 / w[k]));
    }
    return b;
}

// after the first launch of the plan's staged kernel: keep it or go back to the plain one
void FusedAggregationOperator::staged_decide(const Compiled& ck, const uint64_t* slab, int grid, int64_t vec_rows, hipStream_t s)
{
    const KernelInfo& ki = ck.info;
    const int ns = (int)ki.stage_bytes.size() - 1;
    if (staged_mode() != 2 || ns < 1 || vec_rows <= 0 || ck.staged_verdict.load(std::memory_order_relaxed) != 0) return;
    std::vector<uint64_t> cnt((size_t)grid * ns);
    PA_HIP(hipMemcpyAsync(cnt.data(), slab + (size_t)grid * ki.nw, cnt.size() * 8, hipMemcpyDeviceToHost, s));
    PA_HIP(hipStreamSynchronize(s));
    std::vector<double> alive(ns, 0.0);
    for (int b = 0; b < grid; b++) {
        for (int k = 0; k < ns; k++) alive[k] += (double)cnt[(size_t)b * ns + k];
    }
    double eager = 0;
    for (int k = 0; k < ns; k++) alive[k] /= (double)vec_rows;
    for (int w : ki.stage_bytes) eager += w;
    ck.staged_verdict.store(staged_bytes(ki.stage_bytes, alive) <= kStagedGain * eager ? 1 : 2, std::memory_order_relaxed);
}

std::shared_ptr<const FusedAggregationOperator::Compiled> FusedAggregationOperator::shared_lookup(const std::string& key)
{
    std::lock_guard<std::mutex> lock(shared_mutex());
    auto it = shared_cache().find(key);
    return it == shared_cache().end() ? nullptr : it->second;
}

std::mutex& FusedAggregationOperator::shared_mutex()
{
    static std::mutex* m = new std::mutex();
    return *m;
}

std::map<std::string, std::shared_ptr<const FusedAggregationOperator::Compiled>>& FusedAggregationOperator::shared_cache()
{
    static auto* c = new std::map<std::string, std::shared_ptr<const Compiled>>();  // leaked: HIP may be gone at exit
    return *c;
}

const FusedAggregationOperator::Compiled& FusedAggregationOperator::kernel_for(const std::string& sig, const std::vector<ChannelLayout>& layout, int variant)
{
    HostTraceScope trace("    fused.kernel_for");
    std::string key = sig + "|" + std::to_string(variant);
    auto it = compiled_.find(key);
    if (it != compiled_.end()) return *it->second;
    int dev = 0;
    PA_HIP(hipGetDevice(&dev));
    const std::string shared_key = std::to_string(dev) + "|" + key + "|" + plan_fingerprint_;
    if (auto hit = shared_lookup(shared_key)) {
        adopt_layout(*hit);
        compiled_[key] = hit;
        return *hit;
    }
    auto c = std::make_shared<Compiled>();
    c->info = generate(spec_, layout, variant);
    c->kernel = jit_get(c->info.source, c->info.entry);
    if (variant == V_LDS) c->tail_kernel = jit_get(c->info.source, c->info.entry + "_tail");
    if (variant == V_BROW) c->tail_kernel = jit_get(c->info.source, "pa_brow_keys");
    c->kinds.ensure(sizeof(int32_t) * c->info.word_kind.size());
    PA_HIP(hipMemcpyAsync(c->kinds.ptr(), c->info.word_kind.data(), sizeof(int32_t) * c->info.word_kind.size(), hipMemcpyHostToDevice, stream_.get()));
    PA_HIP(hipStreamSynchronize(stream_.get()));
    adopt_layout(*c);
    {
        std::lock_guard<std::mutex> lock(shared_mutex());
        shared_cache()[shared_key] = c;
    }
    const Compiled& ref = *c;
    compiled_[key] = std::move(c);
    return ref;
}

void FusedAggregationOperator::adopt_layout(const Compiled& c)
{
    if (!kinds_dev_) kinds_dev_ = c.kinds.as<int32_t>();
    if (!layout_fixed_) {
        nw_ = c.info.nw;
        w_ = c.info.w;
        layout_id_ = c.info.layout_id;
        layout_fixed_ = true;
    }
    // every signature of one state must yield the same layout: a channel that turns nullable adds count words / NULL
    // flags, and states of different layouts cannot be merged word by word -- the page starts the next generation
    if (c.info.layout_id != layout_id_) throw LayoutChange{};
}

}  // namespace fused_op
}  // namespace pa
