// probe_stage.hpp -- the probe stage on the host: an INNER join over a lookup source with ONE integer key and no duplicate keys, run
// inside another operator's kernel (the fused aggregation: fused_plan.hpp JoinStage; FilterAndProject with the probe inside:
// op_filter_project.cpp).  A probe row finds at most one build row; the build columns the operator wants are "virtual" channels
// n_in + v of its generated code, read at the build position.  The device side is pa_join_probe_* in kernels/pa_device.h, templates
// over the argument block: fill_probe_args is their counterpart here.  Where the probe key lives is the operator's own business.
#pragma once

#include <memory>
#include <ostream>
#include <string>
#include <vector>

#include "exprgen.hpp"
#include "join_source.hpp"
#define PA_ARGS_STDINT
#include "kernels/pa_args.h"

namespace pa {

struct ProbeStage {
    std::shared_ptr<LookupSourceImpl> ls;
    std::vector<int> build_cols;       // virtual channel n_in + v reads ls->rows.cols[build_cols[v]] at the build position
    std::vector<int32_t> build_types;

    // build column `col` becomes a virtual channel: its v.  (What an operator adds is its own choice: the aggregation the columns it
    // reads, FilterAndProject every build output channel.)
    int add_build_column(int col);
    // the expression that reads build column v: an input reference to channel n_in + v
    OwnedExpr build_column_ref(int n_in, int v) const;
    // first page: the build side has published a lookup source this stage can probe
    void require_built() const;
    // the build columns as channels n_in + v behind a page's layout (and 'N' / '_' behind its signature): nullable as the lookup source
    // says -- the never-built shape of a *_source_for_desc path says "not"
    void append_build_channels(std::vector<ChannelLayout>* layout, std::string* sig = nullptr) const;
    // `const T c<n_in + v> = ((const T*)a.bv[v])[jb];` (and cn<n_in + v>) per build column; layout: the page's with the build channels
    void emit_build_loads(std::ostream& out, int n_in, const std::vector<ChannelLayout>& layout) const;
};

// What pa_lookup_join_desc + bridge must say for a probe stage behind a FilterAndProject whose projections have `probe_types`
// (the probe page): INNER, no join filter, one BIGINT / INTEGER / DATE key of the build key's type, channels inside the probe page.
// Returns the probe page's channel that is the join key.
int check_probe_join(const pa_lookup_join_desc& jd, const pa_lookup_source* bridge, const std::vector<int32_t>& probe_types);

// A = PaFusedArgs or PaFpArgs (jrows, which only the former has, is its caller's)
template <class A>
void fill_probe_args(A& a, const ProbeStage& ps)
{
    const LookupSourceImpl& ls = *ps.ls;
    a.jslots = ls.key_slots.ptr();
    a.jmask = ls.probe_mask;
    a.jwrap = ls.probe_wrap;
    a.jbits = ls.bitmap.bits;
    a.jmin = ls.bitmap.min_key;
    a.jrange = ls.bitmap.range;
    a.jrank = reinterpret_cast<const pa_u32x4*>(ls.rank.words);
    a.jrank_rows = ls.rank.rows;
    for (size_t v = 0; v < ps.build_cols.size(); v++) {
        const DevColumn bc = ls.rows.view(ps.build_cols[v]);
        a.bv[v] = bc.values;
        a.bn[v] = bc.nulls;
    }
}

}  // namespace pa
