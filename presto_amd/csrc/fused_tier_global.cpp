// fused_tier_global.cpp -- GLOBAL: no group keys.  Per-lane register accumulators -> wave shuffle -> LDS -> one partial state per
// workgroup in a slab -> fixed-order merge kernel (bitwise reproducible).  (AggregationOperator.addInput,
// …/operator/AggregationOperator.java:145-160, behind the page's filter and projections.)
#include "decimal_host.hpp"
#include "fused_codegen.hpp"
#include "scan_kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <set>

namespace pa {
namespace fused {

void FusedGen::global_declarations()
{
    src << "struct PaAcc {";
    for (int w = 0; w < k.nw; w++) src << (words[w].kind == W_SUMF ? " double" : (words[w].kind == W_MAXU ? " u64" : " i64")) << " w" << w << ";";
    src << " };\n";
}

void FusedGen::global_accumulate_row()
{
    src << "if (sel) {\n";
    for (int w = 0; w < k.nw; w++) {
        if (words[w].kind == W_SUMF) src << "if (" << uflag(w) << ") acc.w" << w << " = acc.w" << w << " + x" << w << ";\n";
        else if (words[w].kind == W_SUMI) src << "if (" << uflag(w) << ") acc.w" << w << " = pa_add_exact(acc.w" << w << ", x" << w << ", a.err);\n";
        else if (words[w].kind == W_MAXU) src << "if (" << uflag(w) << ") acc.w" << w << " = x" << w << " > acc.w" << w << " ? x" << w << " : acc.w" << w << ";\n";
        else src << "if (" << uflag(w) << ") acc.w" << w << " += x" << w << ";\n";
    }
    src << "}\n";
}

void FusedGen::global_kernel_begin()
{
    src << "    PaAcc acc;\n";
    for (int w = 0; w < k.nw; w++) src << "    acc.w" << w << " = 0;\n";
}

void FusedGen::global_thread_ids()
{
    // XCD-aware block -> tile mapping: consecutive workgroup ids go round-robin to the 8 XCDs, so give the
    // workgroups of one XCD consecutive tiles (each XCD's L2 / TLB then walks one contiguous eighth of every grid
    // stride).  Measured on Q6: 0.75 -> 0.79 of the HBM peak; neutral for the one-wave workgroups of the LDS variant.
    src << "    const u32 bsw = (gridDim.x & 7u) == 0u ? (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;\n"
           "    const i64 t = (i64)bsw * " << B << " + threadIdx.x, T = (i64)gridDim.x * " << B << ";\n";
}

void FusedGen::global_kernel_end()
{
    src << "    __shared__ u64 red[" << (B / 64) << " * PA_NW];\n    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;\n";
    for (int w = 0; w < k.nw; w++) {
        if (words[w].kind == W_SUMF) src << "    { double v = pa_wave_sum_f64(acc.w" << w << "); if (lane == 0) red[wave * PA_NW + " << w << "] = (u64)__double_as_longlong(v); }\n";
        else if (words[w].kind == W_SUMI) src << "    { i64 v = pa_wave_sum_i64_exact(acc.w" << w << ", a.err); if (lane == 0) red[wave * PA_NW + " << w << "] = (u64)v; }\n";
        else if (words[w].kind == W_MAXU) src << "    { u64 v = pa_wave_max_u64(acc.w" << w << "); if (lane == 0) red[wave * PA_NW + " << w << "] = v; }\n";
        else src << "    { i64 v = pa_wave_sum_i64(acc.w" << w << "); if (lane == 0) red[wave * PA_NW + " << w << "] = (u64)v; }\n";
    }
    src << "    __syncthreads();\n    if (threadIdx.x < PA_NW) {\n        const int w = threadIdx.x;\n        u64 r = red[w];\n";
    src << "        for (int i = 1; i < " << (B / 64) << "; i++) {\n            u64 o = red[i * PA_NW + w];\n";
    src << "            switch (w) {\n";
    for (int w = 0; w < k.nw; w++) {
        src << "                case " << w << ": ";
        if (words[w].kind == W_SUMF) src << "r = (u64)__double_as_longlong(__longlong_as_double((i64)r) + __longlong_as_double((i64)o)); break;\n";
        else if (words[w].kind == W_SUMI) src << "r = (u64)pa_add_exact((i64)r, (i64)o, a.err); break;\n";
        else if (words[w].kind == W_MAXU) src << "r = o > r ? o : r; break;\n";
        else src << "r = r + o; break;\n";
    }
    src << "            }\n        }\n        a.slab[(u64)blockIdx.x * PA_NW + w] = r;\n    }\n";
    if (staged) {
        // rows that asked for the columns of stages 1 .. n - 1, per workgroup, behind the partial states of all workgroups
        const int ns = s.n_stages - 1;
        src << "    __shared__ u64 pa_scnt[" << (B / 64) << " * " << ns << "];\n";
        for (int k = 1; k <= ns; k++) {
            src << "    { const i64 v = pa_wave_sum_i64((i64)pa_cnt" << k << "); if (lane == 0) pa_scnt[wave * " << ns << " + " << (k - 1) << "] = (u64)v; }\n";
        }
        src << "    __syncthreads();\n    if (threadIdx.x < " << ns << ") {\n        u64 r = 0;\n        for (int i = 0; i < " << (B / 64)
            << "; i++) r += pa_scnt[i * " << ns << " + threadIdx.x];\n"
               "        a.slab[(u64)gridDim.x * PA_NW + (u64)blockIdx.x * " << ns << " + threadIdx.x] = r;\n    }\n";
    }
}

int nt_level()
{
    const char* e = getenv("PRESTO_AMD_NT");
    return e ? std::max(0, std::min(2, atoi(e))) : 1;
}

// ---- V_GLOBAL_S: the staged page loop ----
// Stage k of the plan (Spec::conjunct_begin) evaluates its conjuncts for the rows conjuncts 0 .. begin_k - 1 left alive, and only
// those rows ask for the columns of stage k + 1: a 16-byte load whose rows are all dead reads the column's first quad instead -- one
// hot line -- so that every load is unconditional and the loads of the quads in flight come back in the order they were issued.
void FusedGen::staged_row_functions()
{
    const int S = s.n_stages;
    // the accumulation of the selected rows: pa_row without the filter (`live` is the selection)
    const std::string filtered = body.str();
    body.str("");
    body << "const bool sel = live;\n";
    row_function("pa_row_sel");
    body.str(filtered);
    for (int k = 0; k < S; k++) {
        const int j0 = s.conjunct_begin[k], j1 = k + 1 < S ? s.conjunct_begin[k + 1] : (int)s.conjuncts.size();
        if (j0 >= j1) continue;
        // a conjunct that is FALSE decides the row; a NULL one does not (a later FALSE still makes the AND FALSE, a later error
        // is still raised: AndCodeGenerator's short circuit)
        src << "__device__ __forceinline__ void pa_stage" << k << "(const PaFusedArgs& a, const i32 row" << row_params(ri, layout)
            << ", bool& dead, bool& nul)\n{\n";
        for (int j = j0; j < j1; j++) {
            OwnedExpr sub = s.filter;
            sub.root = s.conjuncts[j];
            std::ostringstream os;
            GenValue v = gen.emit(sub, os);
            src << "if (!dead) {\n" << os.str();
            if (v.nullable()) src << "if (" << v.n << ") nul = true; else if (!(" << v.v << ")) dead = true;\n}\n";
            else src << "if (!(" << v.v << ")) dead = true;\n}\n";
        }
        src << "}\n\n";
    }
    k.stage_bytes.assign(S, 0);
    for (int c = 0; c < s.n_in; c++) {
        if (!s.used_channel[c]) continue;
        k.stage_bytes[s.channel_stage[c]] += type_width(layout[c].type) + (layout[c].nullable ? 1 : 0);
    }
}

void FusedGen::staged_page_loop()
{
    const int S = s.n_stages;
    std::vector<VectorVar> vars;
    vector_load_vars(ri, layout, vars, ColumnNames(), true);
    // per channel: the last stage that reads it (the projections': the last stage)
    std::vector<int> last(s.n_in, -1);
    for (int k = 0; k < S; k++) {
        const int j0 = s.conjunct_begin[k], j1 = k + 1 < S ? s.conjunct_begin[k + 1] : (int)s.conjuncts.size();
        for (int j = j0; j < j1; j++) {
            std::set<int32_t> ch;
            OwnedExpr sub = s.filter;
            sub.root = s.conjuncts[j];
            sub.collect_channels(&ch);
            for (int32_t c : ch) {
                if (c >= 0 && c < s.n_in) last[c] = std::max(last[c], k);
            }
        }
    }
    {
        std::set<int> used_proj;
        for (const auto& ag : s.aggs) {
            if (ag.fn != PA_AGG_COUNT_STAR || s.step == PA_STEP_FINAL) used_proj.insert(ag.input_channel);
            if (s.step == PA_STEP_FINAL && ag.fn != PA_AGG_COUNT && ag.fn != PA_AGG_COUNT_STAR) used_proj.insert(ag.input_channel + 1);
            if (ag.mask_channel >= 0) used_proj.insert(ag.mask_channel);
        }
        std::set<int32_t> ch;
        for (int j : used_proj) s.proj[j].collect_channels(&ch);
        for (int32_t c : ch) {
            if (c >= 0 && c < s.n_in) last[c] = S - 1;
        }
    }
    // conjuncts that may raise an error from stage k on: a NULL row then still goes on (nothing but a FALSE conjunct hides them)
    std::vector<bool> throws_from(S + 1, false);
    for (int k = S - 1; k >= 0; k--) {
        const int j0 = s.conjunct_begin[k], j1 = k + 1 < S ? s.conjunct_begin[k + 1] : (int)s.conjuncts.size();
        bool t = throws_from[k + 1];
        for (int j = j0; j < j1; j++) t = t || gen.can_throw(s.filter, s.conjuncts[j]);
        throws_from[k] = t;
    }
    auto stage_of = [&](const VectorVar& v) { return s.channel_stage[v.channel]; };
    // holder h keeps the quad that stage h works on next: the variables of the channels loaded up to stage h and read from it on
    auto held = [&](const VectorVar& v, int h) { return stage_of(v) <= h && last[v.channel] >= h; };
    auto H = [](int h) { return "h" + std::to_string(h) + "_"; };
    auto args = [&](int h, int r) {
        std::string a;
        for (int c = 0; c < s.n_in; c++) {
            if (!ri.used[c]) continue;
            if (s.channel_stage[c] <= h && last[c] >= h) {
                a += vector_var_channel_args(layout, H(h), r, c);
                continue;
            }
            switch (layout[c].type) {  // (not read at this stage)
                case PA_REAL: a += ", 0.0f"; break;
                case PA_DOUBLE: a += ", 0.0"; break;
                case PA_BOOLEAN: a += ", false"; break;
                case PA_VARCHAR: a += ", (const u8*)0, 0"; break;
                default: a += ", (i64)0"; break;
            }
            if (layout[c].nullable) a += ", false";
        }
        return a;
    };
    // the load of variable v for the quad of holder h, `q` (the rows alive: holder h's flags); rows = the rows of the quad the
    // variable carries.  The 16-byte loads of column values are non-temporal under PRESTO_AMD_NT: from level 1 those of stage 0, which
    // every row asks for, from level 2 also the later stages', whose dead quads re-read one line (both halves of a quad alike)
    const int nt = nt_level();
    auto streamed = [&](const VectorVar& v) {
        return (v.name[0] == 'A' || v.name[0] == 'B') && v.type != "u32" && nt >= (stage_of(v) == 0 ? 1 : 2);
    };
    auto masked_load = [&](const VectorVar& v, int h, const std::string& q) {
        std::string any;
        const int r0 = v.per_quad == 2 ? 2 * v.half : 0, r1 = v.per_quad == 2 ? r0 + 2 : 4;
        for (int r = r0; r < r1; r++) any += (any.empty() ? "" : " || ") + std::string("!") + H(h) + "d" + std::to_string(r);
        const std::string idx = v.per_quad == 2 ? "2 * " + q + (v.half ? " + 1" : "") : (v.per_quad == 0 ? "4 * " + q + " + 4" : q);
        std::string ld = "((const " + v.type + "*)" + v.array + ")[(" + any + ") ? " + idx + " : " + (v.per_quad == 0 ? "4" : "0") + "]";
        // (the element's address is named first, so that the load itself still reads `((const T*)a.v[c])[index];`)
        if (streamed(v)) ld = "({ const " + v.type + "* const pa_p = &" + ld + "; __builtin_nontemporal_load(pa_p); })";
        return v.maybe_null ? "(" + v.array + " ? " + ld + " : 0u)" : ld;
    };
    for (int k = 1; k < S; k++) src << "    u32 pa_cnt" << k << " = 0u;\n";
    src << "    if (nq > 0) {\n      const i64 n_it = t < nq ? (nq - 1 - t) / T + 1 : 0;\n";
    for (int h = 0; h < S; h++) {
        src << "      const i64 " << H(h) << "q = " << (h == 0 ? "t" : "0") << ";\n";
        src << "      bool " << H(h) << "d0 = " << (h == 0 ? "n_it == 0" : "true") << ", " << H(h) << "d1 = " << H(h) << "d0, " << H(h) << "d2 = "
            << H(h) << "d0, " << H(h) << "d3 = " << H(h) << "d0;\n";
        src << "      bool " << H(h) << "n0 = false, " << H(h) << "n1 = false, " << H(h) << "n2 = false, " << H(h) << "n3 = false;\n";
        for (const VectorVar& v : vars) {
            if (held(v, h)) src << "      " << v.type << " " << H(h) << v.name << " = " << masked_load(v, h, H(h) + "q") << ";\n";
        }
    }
    // (the quad of holder h is the lane's quad it - h: the index a row whose quad has rows alive reads)
    src << "      for (i64 it = 0; it < n_it + " << (S - 1) << "; it++) {\n";
    for (int h = 0; h < S; h++) src << "        const i64 " << H(h) << "q = t + (it - " << h << ") * T;\n";
    // the last stage: its conjuncts, then the accumulation of the selected rows (in the order of the plain loop: quad by quad)
    const int L = S - 1;
    for (int r = 0; r < 4; r++) {
        const std::string R = std::to_string(r), row = "(i32)(4 * " + H(L) + "q + " + R + ")";
        if (s.conjunct_begin[L] < (int)s.conjuncts.size()) {
            src << "        pa_stage" << L << "(a, " << row << args(L, r) << ", " << H(L) << "d" << R << ", " << H(L) << "n" << R << ");\n";
        }
        src << "        pa_row_sel(a, acc, !" << H(L) << "d" << R << " && !" << H(L) << "n" << R << ", " << row << args(L, r) << ");\n";
    }
    for (int h = S - 2; h >= 0; h--) {
        const int j0 = s.conjunct_begin[h], j1 = s.conjunct_begin[h + 1];
        src << "        // stage " << h << "\n";
        for (int r = 0; r < 4; r++) {
            const std::string R = std::to_string(r), row = "(i32)(4 * " + H(h) + "q + " + R + ")";
            if (j0 < j1) src << "        pa_stage" << h << "(a, " << row << args(h, r) << ", " << H(h) << "d" << R << ", " << H(h) << "n" << R << ");\n";
            if (!throws_from[h + 1]) src << "        " << H(h) << "d" << R << " = " << H(h) << "d" << R << " || " << H(h) << "n" << R << ";\n";
        }
        const std::string N = H(h + 1), P = H(h);
        // (a NULL conjunct only matters to the rows a later error may still reach: otherwise the row is dead already)
        for (int r = 0; r < 4; r++) {
            src << "        " << N << "d" << r << " = " << P << "d" << r << "; " << N << "n" << r << " = " << (throws_from[h + 1] ? P + "n" + std::to_string(r) : "false") << ";\n";
        }
        src << "        pa_cnt" << (h + 1) << " += (u32)!" << N << "d0 + (u32)!" << N << "d1 + (u32)!" << N << "d2 + (u32)!" << N << "d3;\n";
        for (const VectorVar& v : vars) {
            if (held(v, h + 1) && stage_of(v) <= h) src << "        " << N << v.name << " = " << P << v.name << ";\n";
        }
        for (const VectorVar& v : vars) {
            // (the quad moving on is holder h's: holder h + 1 takes it over in the next iteration)
            if (held(v, h + 1) && stage_of(v) == h + 1) src << "        " << N << v.name << " = " << masked_load(v, h + 1, P + "q") << ";\n";
        }
    }
    // stage 0 of the lane's next quad
    src << "        {\n          const bool ln = it + 1 < n_it;\n          const i64 h0_q = t + (it + 1) * T;\n"
           "          h0_d0 = !ln; h0_d1 = !ln; h0_d2 = !ln; h0_d3 = !ln; h0_n0 = false; h0_n1 = false; h0_n2 = false; h0_n3 = false;\n";
    for (const VectorVar& v : vars) {
        if (held(v, 0)) src << "          h0_" << v.name << " = " << masked_load(v, 0, "h0_q") << ";\n";
    }
    src << "        }\n      }\n    }\n";
}

}  // namespace fused
}  // namespace pa
