"""Packed group keys of the few-groups tier ("Packed keys: a 32-bit key table and the next quad's loads"), off the GPU:
a key that fills one word with at most 31 bits -- the Q1 shape, a nullable (BOOLEAN, VARCHAR(3)) pair with exactly 31 -- generates the
32-bit table preset to a value no key takes and the head loop that loads a quad ahead, and compiles for gfx950 (hiprtc in process);
PRESTO_AMD_LDS_PIPE=0 generates the plain loop under another kernel name.  Keys that are not packed (32 bits, 64 bits, two words)
generate what they generated before: their sources are compared with hashes taken from the parent commit, as
tests/test_codegen_varchar1_unit.py does for its shapes."""
import ctypes as C
import hashlib
import re

import pytest

from presto_amd import abi, tpch
from presto_amd._lib import lib
from presto_amd.expr import field
from presto_amd.operators import fused_aggregation_desc
from tests.test_codegen_varchar1_unit import vector_loops

V_LDS, V_LDS_R = 1, 8
AGGS = [(abi.AGG_SUM, 2, abi.DOUBLE), (abi.AGG_COUNT_STAR, -1, None)]

# name -> (input types, type params, filter, projections, group by, aggregates, nullable channels)
PACKED = {
    "q1": (tpch.Q1_TYPES, tpch.Q1_TYPE_PARAMS, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES, 0),
    # 1 + 1 (NULL flag) + 8 * 3 + 4 + 1 (NULL flag) = 31 bits
    "boolean_varchar3_nullable": ([abi.BOOLEAN, abi.VARCHAR, abi.DOUBLE], [0, 3, 0], None,
                                  [field(0, abi.BOOLEAN), field(1, abi.VARCHAR), field(2, abi.DOUBLE)], [0, 1], AGGS, 0b011),
}
# keys that are not packed -> sha256 of the generated source on the parent commit (of the whole translation unit, so re-taken when the
# device header in front of the generated text changed -- kernels/pa_args.h -- with the generated text byte-identical)
PLAIN = {
    "integer": ([abi.INTEGER, abi.BIGINT, abi.DOUBLE], [0], "dd3f1de13da11ea786efd3641e08906a5cc72b94fdee45976f3424aca8c959b4"),
    "bigint": ([abi.INTEGER, abi.BIGINT, abi.DOUBLE], [1], "ca8d7e90fe773835e3f7c43f78632811cee673f28c08aa9a3ffd31d2cccab195"),
    "two_words": ([abi.INTEGER, abi.BIGINT, abi.DOUBLE], [0, 1], "ba84a9dec53c3a4f57d64557e03de2eb0273819ba52f58112e26c37d7d03569c"),
}


def translation_unit(desc, variant, mask, compile_it=False):
    L = lib()
    L.pa_codegen_fused_layout.restype = C.c_int64
    L.pa_codegen_fused_layout.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_char_p, C.c_int64]
    if compile_it:
        rc = L.pa_codegen_fused_layout(C.byref(desc), variant, mask, 1, None, 0)
        assert rc > 1000, (rc, L.pa_last_error()[-800:])
        return None
    need = L.pa_codegen_fused_layout(C.byref(desc), variant, mask, 0, None, 0)
    assert need > 0, L.pa_last_error()
    buf = C.create_string_buffer(need)
    L.pa_codegen_fused_layout(C.byref(desc), variant, mask, 0, buf, need)
    return buf.value.decode()


def packed_desc(name):
    types, params, flt, proj, gb, aggs, mask = PACKED[name]
    return fused_aggregation_desc(types, flt, proj, gb, aggs, type_params=params), mask


def plain_source(name):
    types, gb, _ = PLAIN[name]
    d, keep = fused_aggregation_desc(types, None, [field(i, t) for i, t in enumerate(types)], gb, AGGS)
    return translation_unit(d, V_LDS, 0)


def kernel_name(src):
    return re.search(r"#define PA_K\(name\) name##_(\w+)", src).group(1)


def head_kernel(src):
    at = src.index("void PA_K(pa_fused_lds)(")
    return src[at:src.index("void PA_K(pa_fused_lds_tail)(")]


@pytest.mark.parametrize("name", sorted(PACKED))
def test_packed_keys_generate_the_32_bit_table_and_the_loop_that_loads_ahead(name, monkeypatch):
    monkeypatch.delenv("PRESTO_AMD_LDS_PIPE", raising=False)
    (d, keep), mask = packed_desc(name)
    for variant in (V_LDS, V_LDS_R):   # (the range-table kernel shares the row function)
        src = translation_unit(d, variant, mask)
        assert "struct PaAcc { u32 tk[PA_C]; int tcount; u32 lane; };" in src
        assert "acc.tk[s] = 0xFFFFFFFFu;" in src
        assert "if (key == acc.tk[s]) g = s;" in src and "s < acc.tcount" not in src
        assert "e[E] = (u64)acc.tk[i];" in src    # the slab's key word stays 64 bits wide
        translation_unit(d, variant, mask, compile_it=True)
    src = translation_unit(d, V_LDS, mask)
    head = head_kernel(src)
    loops = vector_loops(head)
    assert len(loops) == 1
    body = loops[0]
    # the loads of quad q + T are issued, behind their guard, before anything of quad q is worked on
    at = body.index("if (qn < nq) {")
    assert "const i64 qn = q + T;" in body[:at]
    assert at < body.index("u64 S")
    assert at < body.index("pa_row(")
    ahead = body[at:body.index("}", at)]
    assert "(qn)" in ahead and "[q]" not in ahead and "* q" not in ahead
    # ... and those of a lane's first quad in front of the loop, under the same bound
    assert re.search(r"if \(t < nq\) \{\n(?:[^\n]*\(t\)[^\n]*\n)+ *\}\n *for \(i64 q = t; q < nq; q \+= T\)", head)
    # every load of a column sits in one of the two places
    assert all("(qn)" in line or "(t)" in line for line in head.split("\n") if re.search(r"\(\(const pa_\w+\*\)a\.v\[", line))


@pytest.mark.parametrize("name", sorted(PACKED))
def test_the_switch_generates_the_plain_loop_under_another_name(name, monkeypatch):
    (d, keep), mask = packed_desc(name)
    monkeypatch.delenv("PRESTO_AMD_LDS_PIPE", raising=False)
    piped = translation_unit(d, V_LDS, mask)
    monkeypatch.setenv("PRESTO_AMD_LDS_PIPE", "0")
    plain = translation_unit(d, V_LDS, mask)
    translation_unit(d, V_LDS, mask, compile_it=True)
    assert kernel_name(plain) != kernel_name(piped)
    assert "qn" not in head_kernel(plain) and "__builtin_amdgcn_s_waitcnt" not in plain
    assert "struct PaAcc { u32 tk[PA_C]; int tcount; u32 lane; };" in plain    # the key table does not depend on the switch
    # what the two share is the same text: the row function and everything in front of it
    cut = lambda s: re.sub(r"name##_\w+", "name##_", s[:s.index("void PA_K(pa_fused_lds)(")])
    assert cut(plain) == cut(piped)


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_keys_that_are_not_packed_generate_what_they_did(name, monkeypatch):
    for value in (None, "0"):   # (the switch is about packed keys alone)
        if value is None:
            monkeypatch.delenv("PRESTO_AMD_LDS_PIPE", raising=False)
        else:
            monkeypatch.setenv("PRESTO_AMD_LDS_PIPE", value)
        src = plain_source(name)
        assert "u64 tk[PA_C][PA_KW]" in src and "0xFFFFFFFFu;" not in src and "qn" not in head_kernel(src)
        assert hashlib.sha256(src.encode()).hexdigest() == PLAIN[name][2]
