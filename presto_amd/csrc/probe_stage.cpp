// probe_stage.cpp -- see probe_stage.hpp.
#include "probe_stage.hpp"

namespace pa {

int check_probe_join(const pa_lookup_join_desc& jd, const pa_lookup_source* bridge, const std::vector<int32_t>& probe_types)
{
    PA_REQUIRE(bridge != nullptr && bridge->impl != nullptr, PA_ERR_ILLEGAL_STATE, "lookup source has no build operator yet");
    const LookupSourceImpl& ls = *bridge->impl;
    const int n_probe = (int)probe_types.size();
    PA_REQUIRE(jd.join_type == PA_JOIN_INNER, PA_ERR_NOT_SUPPORTED, "the fused probe is an inner join");
    PA_REQUIRE(jd.filter == nullptr, PA_ERR_NOT_SUPPORTED, "a join filter function runs in the LookupJoinOperator, not in the fused probe");
    PA_REQUIRE(jd.probe_channel_count == n_probe, PA_ERR_INVALID_ARGUMENT, "the probe page is the projection output");
    PA_REQUIRE(jd.join_channel_count == 1 && ls.join_channels.size() == 1, PA_ERR_NOT_SUPPORTED, "the fused probe takes one join key");
    const int kc = jd.probe_join_channels[0];
    PA_REQUIRE(kc >= 0 && kc < n_probe, PA_ERR_INVALID_ARGUMENT, "probe join channel out of range");
    const int32_t kt = probe_types[(size_t)kc];
    PA_REQUIRE(kt == PA_BIGINT || kt == PA_INTEGER || kt == PA_DATE, PA_ERR_NOT_SUPPORTED, "the fused probe takes a BIGINT / INTEGER / DATE key");
    PA_REQUIRE(kt == ls.rows.cols[(size_t)ls.join_channels[0]].type, PA_ERR_INVALID_ARGUMENT, "probe / build join key types differ");
    for (int32_t i = 0; i < jd.probe_output_channel_count; i++) {
        const int c = jd.probe_output_channels[i];
        PA_REQUIRE(c >= 0 && c < n_probe, PA_ERR_INVALID_ARGUMENT, "probe output channel out of range");
    }
    return kc;
}

int ProbeStage::add_build_column(int col)
{
    const int32_t t = ls->rows.cols[(size_t)col].type;
    // (said when the operator is created, not by the code generator at the first page: such a join runs as the operator chain)
    PA_REQUIRE(t != PA_VARCHAR, PA_ERR_NOT_SUPPORTED, "VARCHAR build columns are not read by the fused probe");
    PA_REQUIRE(t != PA_DECIMAL && t != PA_LONG_DECIMAL, PA_ERR_NOT_SUPPORTED, "DECIMAL build columns are not read by the fused probe");
    PA_REQUIRE((int)build_cols.size() < PA_MAX_BUILD_CHANNELS, PA_ERR_NOT_SUPPORTED, "the fused probe reads at most 8 build columns");
    build_cols.push_back(col);
    build_types.push_back(t);
    return (int)build_cols.size() - 1;
}

OwnedExpr ProbeStage::build_column_ref(int n_in, int v) const
{
    OwnedExpr e;
    pa_expr_node node{};
    node.kind = PA_EXPR_INPUT_REF;
    node.type = build_types[(size_t)v];
    node.channel = n_in + v;
    e.nodes.push_back(node);
    e.strings.emplace_back();
    e.root = 0;
    return e;
}

void ProbeStage::require_built() const
{
    PA_REQUIRE(ls->built.load(), PA_ERR_ILLEGAL_STATE, "probe page before the lookup source was built");
    if (int32_t e = ls->error.load()) throw Error(e, "hash build failed on device");
    PA_REQUIRE(ls->keyed && !ls->has_duplicates, PA_ERR_ILLEGAL_STATE, "internal: fused probe over a lookup source with duplicate keys");
}

void ProbeStage::append_build_channels(std::vector<ChannelLayout>* layout, std::string* sig) const
{
    for (size_t v = 0; v < build_cols.size(); v++) {
        ChannelLayout cl;
        cl.type = build_types[v];
        cl.nullable = ls->rows.cols[(size_t)build_cols[v]].has_nulls;  // fixed since the build
        layout->push_back(cl);
        if (sig) *sig += cl.nullable ? 'N' : '_';
    }
}

void ProbeStage::emit_build_loads(std::ostream& out, int n_in, const std::vector<ChannelLayout>& layout) const
{
    for (size_t v = 0; v < build_cols.size(); v++) {
        const std::string id = std::to_string(n_in + (int)v), V = std::to_string(v);
        const int32_t t = build_types[v];
        out << "const " << RowCodegen::ctype(t) << " c" << id << " = ";
        if (t == PA_BIGINT) out << "((const i64*)a.bv[" << V << "])[jb];\n";
        else if (t == PA_INTEGER || t == PA_DATE) out << "(i64)((const i32*)a.bv[" << V << "])[jb];\n";
        else if (t == PA_DOUBLE) out << "((const double*)a.bv[" << V << "])[jb];\n";
        else if (t == PA_REAL) out << "((const float*)a.bv[" << V << "])[jb];\n";
        else if (t == PA_BOOLEAN) out << "((const u8*)a.bv[" << V << "])[jb] != 0;\n";
        else throw Error(PA_ERR_NOT_SUPPORTED, "build column type not read by the fused probe");
        if (layout[(size_t)n_in + v].nullable) out << "const bool cn" << id << " = a.bn[" << V << "] != nullptr && a.bn[" << V << "][jb] != 0;\n";
    }
}

}  // namespace pa
