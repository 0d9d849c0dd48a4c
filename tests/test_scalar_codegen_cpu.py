"""LIKE, substr, length and year / month / day in the expression generator (csrc/exprgen.cpp), without a GPU: every new operator and every
LIKE shape generates and compiles for gfx950 (hiprtc in process), the constant pattern decides the code, and every invalid-argument /
refusal rule of include/presto_amd.h's pa_call_op comment returns its status from the generator -- before a device is asked for."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.expr import and_, call, coalesce, constant, day, field, if_, length, month, substr, year
from presto_amd.operators import _filter_project_desc, fused_aggregation_desc, fused_join_aggregation_desc, hash_builder_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_GLOBAL, V_LDS, V_GT, V_STAGED = 0, 1, 2, 9
TYPES = [abi.VARCHAR, abi.DATE, abi.BIGINT]
S, D, B = field(0, abi.VARCHAR), field(1, abi.DATE), field(2, abi.BIGINT)

LIKE_SHAPES = {
    "equality": S.like("PROMO"), "prefix": S.like("PROMO%"), "suffix": S.like("%BRASS"), "contains": S.like("%green%"),
    "chain": S.like("ab%cd%ef"), "general": S.like("%a_b%"), "escape": S.like("50#%%", "#"), "escape_general": S.like("_#_%", "#"),
}
OTHER_OPS = {
    "substr2": substr(S, B).eq(constant("ab", abi.VARCHAR)), "substr3": substr(S, 1, 2).isin("13", "31"), "length": length(S) > 3,
    "year": year(D).eq(1995), "month": month(D) < 7, "day": day(D).between(1, 15),
    "nested": length(substr(substr(S, 2), -3, 2)).eq(2), "substr_like": substr(S, 2, 5).like("%a_"), "substr_is_null": substr(S, B, B).is_null_(),
}


def fp_source(filter_expr, projections=(), types=TYPES):
    """(generated source behind the device header, kernel key) or (negative status, message)"""
    fp, keep = _filter_project_desc(types, filter_expr, list(projections), abi.MEM_HOST, None)
    L = lib()
    need = L.pa_codegen_filter_project(C.byref(fp), None, 0, None)
    if need < 0:
        return need, L.pa_last_error().decode()
    buf, key = C.create_string_buffer(need), C.create_string_buffer(32)
    L.pa_codegen_filter_project(C.byref(fp), buf, need, key)
    src = buf.value.decode()
    return src[src.index("#define PA_K("):], key.value.decode()


def fp_compile(filter_expr, projections=(), types=TYPES):
    fp, keep = _filter_project_desc(types, filter_expr, list(projections), abi.MEM_HOST, None)
    return lib().pa_codegen_compile_filter_project(C.byref(fp))


def status(filter_expr, projections=(), types=TYPES):
    rc, _ = fp_source(filter_expr, projections, types)
    return rc if isinstance(rc, int) else abi.OK


@pytest.mark.parametrize("name", sorted(LIKE_SHAPES) + sorted(OTHER_OPS))
def test_filter_project_compiles_for_gfx950(name):
    expr = {**LIKE_SHAPES, **OTHER_OPS}[name]
    assert fp_compile(expr, [B]) > 1000, lib().pa_last_error()


def test_boolean_and_bigint_results_are_projections():
    assert fp_compile(None, [S.like("%a_b%"), S.like("ab%cd%ef"), length(S), year(D), month(D), day(D), length(substr(S, B))]) > 1000, lib().pa_last_error()


def test_the_constant_pattern_decides_the_code():
    """specialisation, by function name: only a pattern with `_` reaches the general matcher"""
    want = {"equality": "pa_str_eq(", "prefix": "pa_str_prefix(", "suffix": "pa_str_suffix(", "contains": "pa_str_find(", "escape": "pa_str_prefix("}
    for name, fn in want.items():
        src, _ = fp_source(LIKE_SHAPES[name])
        assert fn in src and "pa_like_general" not in src, name
    src, _ = fp_source(LIKE_SHAPES["prefix"])
    assert "pa_str_find(" not in src and "pa_str_suffix(" not in src
    chain, _ = fp_source(LIKE_SHAPES["chain"])
    assert "pa_str_prefix(" in chain and "pa_str_suffix(" in chain and chain.count("pa_str_find(") == 1 and "cl0 >= 4" in chain and "pa_like_general" not in chain
    for name in ("general", "escape_general"):
        assert "pa_like_general(" in fp_source(LIKE_SHAPES[name])[0]
    # the escaped `%` is a literal byte of the prefix, `%` alone matches everything, `%%` is `%`
    assert '"\\065\\060\\045", 3' in fp_source(LIKE_SHAPES["escape"])[0]
    assert fp_source(S.like("%%"))[0] == fp_source(S.like("%"))[0]


def test_patterns_are_part_of_the_kernel_key():
    (s1, k1), (s2, k2), (s3, k3) = fp_source(S.like("PROMO%")), fp_source(S.like("PROMO%")), fp_source(S.like("PROMA%"))
    assert k1 == k2 and s1 == s2 and k1 != k3
    assert fp_source(S.like("a_c"))[1] != fp_source(S.like("a_d"))[1]
    assert fp_source(year(D).eq(1995))[1] != fp_source(month(D).eq(1995))[1]


def fused_filter():
    return and_(S.like("ab%cd%ef"), year(D).eq(1995))


@pytest.mark.parametrize("variant", [V_GLOBAL, V_STAGED, V_LDS, V_GT], ids=["global", "staged", "lds", "gt"])
def test_fused_tiers_compile_with_a_like_filter(variant):
    grouped = variant in (V_LDS, V_GT)
    for flt in (fused_filter(), and_(S.like("%a_b%"), year(D).eq(1995))):
        d, keep = fused_aggregation_desc(TYPES, flt, [B], [0] if grouped else [], [(abi.AGG_COUNT_STAR, -1, None)])
        L = lib()
        L.pa_codegen_fused_layout.restype = C.c_int64
        L.pa_codegen_fused_layout.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_char_p, C.c_int64]
        for mask in (0, 0b111):
            assert L.pa_codegen_fused_layout(C.byref(d), variant, mask, 1, None, 0) > 1000, (variant, mask, L.pa_last_error())


def test_fused_join_compiles_with_a_like_in_the_probe_filter():
    build, kb = hash_builder_desc([abi.BIGINT, abi.BIGINT], [0], [1])
    d, keep = fused_join_aggregation_desc(TYPES, fused_filter(), [B], [0], [0], [abi.BIGINT, abi.BIGINT], [0], [(abi.AGG_COUNT_STAR, -1, None)])
    assert lib().pa_codegen_compile_fused_join(C.byref(d), C.byref(build), -1) > 1000, lib().pa_last_error()


def V(s): return constant(s, abi.VARCHAR)


INVALID = {
    "like_one_argument": call(abi.OP_LIKE, abi.BOOLEAN, S),
    "like_four_arguments": call(abi.OP_LIKE, abi.BOOLEAN, S, V("a"), V("#"), V("#")),
    "like_value_not_varchar": call(abi.OP_LIKE, abi.BOOLEAN, B, V("a")),
    "like_pattern_not_varchar": call(abi.OP_LIKE, abi.BOOLEAN, S, constant(1, abi.BIGINT)),
    "like_escape_two_characters": S.like("a", "##"),
    "like_escape_not_bmp": S.like("a", "\U0001F600"),
    "like_escape_before_other": S.like("abc#abc", "#"),
    "like_escape_alone": S.like("#", "#"),
    "like_escape_at_end": S.like("abc#", "#"),
    "substr_one_argument": call(abi.OP_SUBSTR, abi.VARCHAR, S).is_null_(),
    "substr_four_arguments": call(abi.OP_SUBSTR, abi.VARCHAR, S, B, B, B).is_null_(),
    "substr_value_not_varchar": call(abi.OP_SUBSTR, abi.VARCHAR, B, B).is_null_(),
    "substr_start_double": call(abi.OP_SUBSTR, abi.VARCHAR, S, constant(1.0, abi.DOUBLE)).is_null_(),
    "substr_length_varchar": call(abi.OP_SUBSTR, abi.VARCHAR, S, B, S).is_null_(),
    "length_two_arguments": call(abi.OP_LENGTH, abi.BIGINT, S, S) > 1,
    "length_not_varchar": call(abi.OP_LENGTH, abi.BIGINT, B) > 1,
    "year_not_date": year(B).eq(1), "month_varchar": month(S).eq(1), "day_two_arguments": call(abi.OP_DAY, abi.BIGINT, D, D).eq(1),
}
REFUSED = {
    "like_pattern_is_a_column": call(abi.OP_LIKE, abi.BOOLEAN, S, S),
    "like_pattern_is_an_expression": call(abi.OP_LIKE, abi.BOOLEAN, S, substr(V("abc"), 1)),
    "like_escape_is_a_column": call(abi.OP_LIKE, abi.BOOLEAN, S, V("a"), S),
    "substr_integer_start": call(abi.OP_SUBSTR, abi.VARCHAR, S, constant(1, abi.INTEGER)).is_null_(),   # the planner casts to BIGINT
    "unknown_operator": call(20, abi.BIGINT, B) > 1,
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_arguments(name):
    assert status(INVALID[name]) == abi.ERR_INVALID_ARGUMENT, lib().pa_last_error()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals(name):
    assert status(REFUSED[name]) == abi.ERR_NOT_SUPPORTED, lib().pa_last_error()


def test_an_empty_escape_disables_escaping_and_null_constants_give_null():
    assert status(S.like("abc#abc", "")) == abi.OK
    for expr in (S.like(constant(None, abi.VARCHAR)), S.like("a", constant(None, abi.VARCHAR)), S.like(constant(None, abi.VARCHAR), "#")):
        src, _ = fp_source(expr)
        assert "pa_str" not in src and "pa_like" not in src
    # a NULL pattern is NULL before the escape rules are looked at; a bad pattern next to a NULL escape likewise
    assert status(S.like("abc#", constant(None, abi.VARCHAR))) == abi.OK


def test_varchar_valued_roots_keys_and_forms_stay_refused():
    sub = substr(S, 2)
    assert status(None, [sub]) == abi.ERR_NOT_SUPPORTED                                   # a VARCHAR projection is a plain input reference
    assert status(if_(B > 1, sub, S).eq(V("a"))) == abi.ERR_NOT_SUPPORTED
    assert status(coalesce(sub, S).eq(V("a"))) == abi.ERR_NOT_SUPPORTED
    d, keep = fused_aggregation_desc(TYPES, None, [sub, B], [0], [(abi.AGG_COUNT_STAR, -1, None)])
    assert lib().pa_codegen_compile_fused(C.byref(d), -1) == abi.ERR_NOT_SUPPORTED      # GROUP BY substr(...)
    assert b"group keys" in lib().pa_last_error()
    d, keep = fused_aggregation_desc(TYPES, None, [sub], [], [(abi.AGG_MAX, 0, abi.VARCHAR)])
    assert lib().pa_codegen_compile_fused(C.byref(d), -1) == abi.ERR_NOT_SUPPORTED


ENUMS = [("PA_OP_CAST", abi.OP_CAST, 13), ("PA_OP_LIKE", abi.OP_LIKE, 14), ("PA_OP_SUBSTR", abi.OP_SUBSTR, 15), ("PA_OP_LENGTH", abi.OP_LENGTH, 16),
         ("PA_OP_YEAR", abi.OP_YEAR, 17), ("PA_OP_MONTH", abi.OP_MONTH, 18), ("PA_OP_DAY", abi.OP_DAY, 19)]


def test_enum_values_match_the_header():
    """the enumerators, printed by a C program compiled against include/presto_amd.h"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "enums.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            for name, _, _ in ENUMS:
                f.write('    printf("%%d\\n", (int)%s);\n' % name)
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "enums")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [v for _, v, _ in ENUMS] == [v for _, _, v in ENUMS]


def test_the_cpp_mirror_and_the_java_serializer_know_the_functions():
    hpp = open(os.path.join(ROOT, "include", "presto_amd.hpp")).read()
    for name in ("like(", "substr(", "length(", "year(", "month(", "day("):
        assert "inline Expr " + name in hpp, name
    java = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "RowExpressionSerializer.java")).read()
    for name, _, value in ENUMS[1:]:
        assert "%s = %d" % (name[3:], value) in java, name
