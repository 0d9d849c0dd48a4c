"""CPU-side checks of the nested-loop join (pa_nested_loop_build_create / pa_nested_loop_join_create): exported, the ctypes mirrors laid
out as the header lays them out, every invalid argument and every refusal of the contract reported at creation -- an invalid argument
before a refusal, both before the device is asked for --, no device -> a loud PA_ERR_NO_DEVICE, the generated pair kernels (source
shape, both lane mappings, compiled for gfx950 through hiprtc), and the model the GPU tests compare against pinned by hand.

A join operator needs a builder on its handle for the build types, and without a device no builder can be made: what the join checks
with the build types in hand is reached here through pa_codegen_nested_loop, which runs the same checks over a build descriptor."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.expr import and_, call, constant, field, or_
from presto_amd.operators import (NestedLoopBuildOperatorFactory, NestedLoopJoinBridge, NestedLoopJoinOperatorFactory, nested_loop_build_desc,
                                  nested_loop_join_desc)
from tests import expr_model as M
from tests import nested_loop_model as NL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_FIELDS = ["input_channel_count", "input_types", "input_type_params", "stream"]
JOIN_FIELDS = ["probe_channel_count", "probe_types", "probe_type_params", "probe_output_channel_count", "probe_output_channels",
               "build_output_channel_count", "build_output_channels", "filter", "output_mem", "stream"]
CARRIED = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, abi.decimal(12, 2), abi.decimal(30, 2)]
TRUE = constant(True, abi.BOOLEAN)


def has_gpu():
    return lib().pa_device_count() > 0


def lt(a, b):
    return call(abi.OP_LESS_THAN, abi.BOOLEAN, a, b)


def create(factory, bridge):
    h = C.c_void_p()
    return factory._create(C.byref(factory._desc), bridge._h, C.byref(h))


def codegen(probe_types, probe_out, build_types, build_out, filter_expr, variant=0, compile=False, **kw):
    """status (negative) or the source of the pair kernels / the size of their code object"""
    jd, k1 = nested_loop_join_desc(probe_types, probe_out, build_out, filter_expr, **kw)
    bd, k2 = nested_loop_build_desc(build_types)
    L = lib()
    if compile:
        return L.pa_codegen_compile_nested_loop(C.byref(jd), C.byref(bd), variant)
    need = L.pa_codegen_nested_loop(C.byref(jd), C.byref(bd), variant, None, 0)
    if need < 0:
        return need
    buf = C.create_string_buffer(need)
    assert L.pa_codegen_nested_loop(C.byref(jd), C.byref(bd), variant, buf, need) == need
    return buf.value.decode()


def test_entry_points_are_exported():
    L = lib()
    for name in ["pa_nested_loop_pages_create", "pa_nested_loop_pages_destroy", "pa_nested_loop_pages_rows", "pa_nested_loop_build_create",
                 "pa_nested_loop_join_create", "pa_codegen_nested_loop", "pa_codegen_compile_nested_loop"]:
        assert getattr(L, name) is not None
    from presto_amd.operators import NestedLoopBuildOperator, NestedLoopJoinOperator   # noqa: F401  (the Python mirrors)


def test_ctypes_layout_matches_the_header():
    """sizeof / offsetof of the two descriptors, printed by a C program compiled against include/presto_amd.h."""
    structs = [("pa_nested_loop_build_desc", BUILD_FIELDS, abi.pa_nested_loop_build_desc), ("pa_nested_loop_join_desc", JOIN_FIELDS, abi.pa_nested_loop_join_desc)]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            for struct, fields, _ in structs:
                f.write('    printf("%%d\\n", (int)sizeof(%s));\n' % struct)
                for name in fields:
                    f.write('    printf("%%d\\n", (int)offsetof(%s, %s));\n' % (struct, name))
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, fields, cls in structs:
        assert [name for name, _ in cls._fields_] == fields
        want += [C.sizeof(cls)] + [getattr(cls, name).offset for name in fields]
    assert got == want


def test_pages_handle_without_a_builder():
    bridge = NestedLoopJoinBridge()
    n = C.c_int64()
    assert lib().pa_nested_loop_pages_rows(bridge._h, C.byref(n)) == abi.ERR_ILLEGAL_STATE
    assert lib().pa_nested_loop_pages_rows(None, C.byref(n)) == abi.ERR_INVALID_ARGUMENT
    # a join needs the build types: no builder on the handle yet
    assert create(NestedLoopJoinOperatorFactory([abi.BIGINT], [0], []), bridge) == abi.ERR_ILLEGAL_STATE
    assert create(NestedLoopJoinOperatorFactory([abi.BIGINT], [0], [], filter=lt(field(0, abi.BIGINT), field(0, abi.BIGINT))), bridge) == abi.ERR_ILLEGAL_STATE
    bridge.destroy()
    assert lib().pa_nested_loop_pages_destroy(None) == abi.OK


def test_builder_descriptor_checks():
    bridge = NestedLoopJoinBridge()
    L = lib()
    h = C.c_void_p()
    assert L.pa_nested_loop_build_create(None, bridge._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    d, keep = nested_loop_build_desc([abi.BIGINT])
    assert L.pa_nested_loop_build_create(C.byref(d), bridge._h, None) == abi.ERR_INVALID_ARGUMENT
    d.input_channel_count = -1
    assert L.pa_nested_loop_build_create(C.byref(d), bridge._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    d.input_channel_count = 1
    d.input_types = None
    assert L.pa_nested_loop_build_create(C.byref(d), bridge._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    for bad in (-1, 10, 99):
        assert create(NestedLoopBuildOperatorFactory([abi.BIGINT, bad]), bridge) == abi.ERR_INVALID_ARGUMENT, bad
    assert create(NestedLoopBuildOperatorFactory([abi.BIGINT, abi.ROW]), bridge) == abi.ERR_NOT_SUPPORTED
    assert create(NestedLoopBuildOperatorFactory([abi.BIGINT] * 65), bridge) == abi.ERR_NOT_SUPPORTED
    # an invalid argument before a refusal
    assert create(NestedLoopBuildOperatorFactory([abi.ROW, 99]), bridge) == abi.ERR_INVALID_ARGUMENT
    assert create(NestedLoopBuildOperatorFactory([abi.BIGINT] * 65 + [99]), bridge) == abi.ERR_INVALID_ARGUMENT
    if not has_gpu():
        # a failed creation leaves the handle without a builder
        assert create(NestedLoopJoinOperatorFactory([abi.BIGINT], [0], []), bridge) == abi.ERR_ILLEGAL_STATE


def test_join_descriptor_checks_that_need_no_build_types():
    """... come before the handle is looked at"""
    bridge = NestedLoopJoinBridge()
    L = lib()
    h = C.c_void_p()
    assert L.pa_nested_loop_join_create(None, bridge._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    d, keep = nested_loop_join_desc([abi.BIGINT], [0], [])
    assert L.pa_nested_loop_join_create(C.byref(d), bridge._h, None) == abi.ERR_INVALID_ARGUMENT
    assert L.pa_nested_loop_join_create(C.byref(d), None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    for name in ("probe_channel_count", "probe_output_channel_count", "build_output_channel_count"):
        d, keep = nested_loop_join_desc([abi.BIGINT], [0], [0])
        setattr(d, name, -1)
        assert L.pa_nested_loop_join_create(C.byref(d), bridge._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT, name
    for name in ("probe_types", "probe_output_channels", "build_output_channels"):
        d, keep = nested_loop_join_desc([abi.BIGINT], [0], [0])
        setattr(d, name, None)
        assert L.pa_nested_loop_join_create(C.byref(d), bridge._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT, name
    for channel in (-1, 1, 7):
        assert create(NestedLoopJoinOperatorFactory([abi.BIGINT], [channel], []), bridge) == abi.ERR_INVALID_ARGUMENT, channel
    for mem in (-1, 2):
        assert create(NestedLoopJoinOperatorFactory([abi.BIGINT], [0], [], output_mem=mem), bridge) == abi.ERR_INVALID_ARGUMENT, mem
    for bad in (-1, 10, 99):
        assert create(NestedLoopJoinOperatorFactory([abi.BIGINT, bad], [0], []), bridge) == abi.ERR_INVALID_ARGUMENT, bad
    # ... also where the descriptor holds something the device path refuses
    assert create(NestedLoopJoinOperatorFactory([abi.ROW, 99], [0], []), bridge) == abi.ERR_INVALID_ARGUMENT
    assert create(NestedLoopJoinOperatorFactory([abi.ROW], [], [], output_mem=5), bridge) == abi.ERR_INVALID_ARGUMENT


def test_join_checks_with_the_build_types():
    """pa_codegen_nested_loop runs the join's checks over a build descriptor: the invalid arguments, then the refusals."""
    one = [abi.BIGINT]
    x, y = field(1, abi.BIGINT), field(0, abi.BIGINT)    # p.x is channel B + 0 = 1 of the pair, b.y channel 0
    assert isinstance(codegen(one, [0], one, [0], lt(x, y)), str)
    # invalid: build output channel out of range, a filter that is not BOOLEAN, a filter channel outside the pair
    for channel in (-1, 1):
        assert codegen(one, [0], one, [channel], TRUE) == abi.ERR_INVALID_ARGUMENT
    assert codegen(one, [0], one, [0], call(abi.OP_ADD, abi.BIGINT, x, y)) == abi.ERR_INVALID_ARGUMENT
    for channel in (-1, 2, 9):
        assert codegen(one, [0], one, [0], lt(field(channel, abi.BIGINT), y)) == abi.ERR_INVALID_ARGUMENT, channel
    assert codegen(one, [0], [abi.BIGINT, 99], [0], TRUE) == abi.ERR_INVALID_ARGUMENT
    for variant in (-1, 4):
        assert codegen(one, [0], one, [0], TRUE, variant=variant) == abi.ERR_INVALID_ARGUMENT
    assert codegen(one, [0], one, [0], None) == abi.ERR_INVALID_ARGUMENT      # no filter: no generated kernel
    # refused: PA_ROW anywhere, no output channel at all, more than 64 channels together, what FilterAndProject's filter refuses
    assert codegen([abi.BIGINT, abi.ROW], [0], one, [0], TRUE) == abi.ERR_NOT_SUPPORTED
    assert codegen(one, [0], [abi.ROW, abi.BIGINT], [1], TRUE) == abi.ERR_NOT_SUPPORTED
    assert codegen(one, [], one, [], TRUE) == abi.ERR_NOT_SUPPORTED
    assert codegen([abi.BIGINT] * 40, [0], [abi.BIGINT] * 25, [0], TRUE) == abi.ERR_NOT_SUPPORTED
    assert isinstance(codegen([abi.BIGINT] * 40, [0], [abi.BIGINT] * 24, [0], TRUE), str)
    mixed = lt(field(1, abi.DOUBLE), field(0, abi.BIGINT))          # DOUBLE against BIGINT needs an explicit CAST
    assert codegen([abi.DOUBLE], [0], one, [0], mixed) == abi.ERR_NOT_SUPPORTED
    fp, keep = __import__("presto_amd.operators", fromlist=["_filter_project_desc"])._filter_project_desc([abi.BIGINT, abi.DOUBLE], mixed, [], abi.MEM_HOST, None)
    assert lib().pa_codegen_filter_project(C.byref(fp), None, 0, None) == abi.ERR_NOT_SUPPORTED       # ... the same status
    # an invalid argument before a refusal
    assert codegen([abi.ROW], [0], one, [5], TRUE) == abi.ERR_INVALID_ARGUMENT
    assert codegen([abi.ROW], [0], one, [0], lt(field(7, abi.BIGINT), y)) == abi.ERR_INVALID_ARGUMENT
    assert codegen(one, [], one, [], call(abi.OP_ADD, abi.BIGINT, x, y)) == abi.ERR_INVALID_ARGUMENT
    # every carried type is taken on either side
    for t in CARRIED:
        assert isinstance(codegen([t], [0], [t], [0], TRUE), str), t


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    bridge = NestedLoopJoinBridge()
    assert create(NestedLoopBuildOperatorFactory(CARRIED), bridge) == abi.ERR_NO_DEVICE
    assert create(NestedLoopBuildOperatorFactory([]), bridge) == abi.ERR_NO_DEVICE
    assert b"no" in lib().pa_last_error().lower()


# ---- generated source -------------------------------------------------------------------------------------------------------------------
# build page (y BIGINT, d DOUBLE, s VARCHAR, unread BIGINT), probe page (x BIGINT, e DOUBLE, t VARCHAR, unread INTEGER)
BT = [abi.BIGINT, abi.DOUBLE, abi.VARCHAR, abi.BIGINT]
PT = [abi.BIGINT, abi.DOUBLE, abi.VARCHAR, abi.INTEGER]
MIXED = and_(lt(field(4, abi.BIGINT), field(0, abi.BIGINT)), or_(lt(field(1, abi.DOUBLE), field(5, abi.DOUBLE)),
                                                                  call(abi.OP_EQUAL, abi.BOOLEAN, field(2, abi.VARCHAR), field(6, abi.VARCHAR))))
KERNELS = {0: ("pa_nl_count_rows", "pa_nl_emit_rows"), 1: ("pa_nl_count_build", "pa_nl_emit_build")}


def body_of(source, kernel):
    """the text of one generated kernel"""
    at = source.index("PA_K(%s)" % kernel)
    end = source.find('extern "C"', at)
    return source[at:end if end >= 0 else len(source)]


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_generated_source(variant):
    source = codegen(PT, [0, 3], BT, [3], MIXED, variant=variant)
    source = source[source.index("#define PA_K("):]       # (behind the device header)
    lanes, nullable = variant & 1, bool(variant & 2)
    count, emit = KERNELS[lanes]
    other = KERNELS[1 - lanes]
    # each variant has its own kernel names, a count form and an emit form
    assert "PA_K(%s)" % count in source and "PA_K(%s)" % emit in source
    assert other[0] not in source and other[1] not in source
    # the predicate is written once and both forms call it
    assert source.count("bool pa_nl_keep(") == 1
    assert "pa_nl_keep(a" in body_of(source, count) and "pa_nl_keep(a" in body_of(source, emit)
    strip = lambda s: re.sub(r"\s+", " ", s)
    call_of = lambda body: strip(body[body.index("pa_nl_keep(a"):body.index(")) {" if lanes == 0 else ");", body.index("pa_nl_keep(a"))])
    assert call_of(body_of(source, count)) == call_of(body_of(source, emit))
    # only the channels the filter reads are loaded: pair channels 0, 1, 2 (build) and 4, 5, 6 (probe); 3 and 7 appear nowhere
    for c in (0, 1, 2, 4, 5, 6):
        assert "a.v[%d]" % c in source, c
    for c in (3, 7):
        assert "a.v[%d]" % c not in source and "a.o[%d]" % c not in source and "a.nl[%d]" % c not in source and not re.search(r"\bc%d\b" % c, source), c
    # VARCHAR operands come in as (pointer, length) from the offsets
    assert "a.o[2]" in source and "a.o[6]" in source and "i32 cl2" in source and "i32 cl6" in source
    # NULL flags are loaded only for channels that have them
    assert ("a.nl[0]" in source) == nullable and ("bool cn4" in source) == nullable
    # what decides a position: the scanned offsets, never an atomic
    assert "atomicAdd" not in source
    assert "a.offsets[pa_r]" in body_of(source, emit) and "a.counts[pa_r]" in body_of(source, count)
    if lanes == 0:
        assert "__shared__" in source and "__syncthreads()" in source     # the build's filter channels come through LDS
    else:
        assert "__ballot(" in source and "__popcll(" in source


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_generated_source_compiles_for_gfx950(variant):
    size = codegen(PT, [0, 3], BT, [3], MIXED, variant=variant, compile=True)
    assert size > 0, lib().pa_last_error().decode()


def test_wide_build_rows_are_not_staged():
    """more build bytes per row than one LDS chunk holds: variant 0 reads them from memory (and still compiles)"""
    ld = abi.decimal(30, 2)
    f = and_(*[call(abi.OP_EQUAL, abi.BOOLEAN, field(c, ld), field(c, ld)) for c in range(4)])
    source = codegen([abi.BIGINT], [0], [ld] * 4, [0], f, variant=0)
    assert "__shared__" not in source[source.index("#define PA_K("):]
    assert codegen([abi.BIGINT], [0], [ld] * 4, [0], f, variant=0, compile=True) > 0
    narrow = codegen([abi.BIGINT], [0], [ld] * 2, [0], and_(*[call(abi.OP_EQUAL, abi.BOOLEAN, field(c, ld), field(c, ld)) for c in range(2)]), variant=0)
    assert "__shared__" in narrow[narrow.index("#define PA_K("):]


def test_sources_and_build_list():
    makefile = open(os.path.join(ROOT, "presto_amd", "csrc", "Makefile")).read()
    assert "op_nested_loop.cpp" in makefile and "nested_loop_kernels.hip" in makefile
    kernels = open(os.path.join(ROOT, "presto_amd", "csrc", "nested_loop_kernels.hpp")).read()
    assert re.search(r"kNestedLoopLdsChunk\s*=\s*\d+", kernels) and "launch_nested_loop_product(" in kernels


def test_jni_shim_and_java_natives():
    """jni/presto_amd_jni.c compiles against the stand-in jni.h and exports the four natives GpuNative.java declares"""
    shim = os.path.join(ROOT, "jni", "presto_amd_jni.c")
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "shim.o")
        subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-fPIC", "-I" + os.path.join(ROOT, "jni", "stub"), "-I" + os.path.join(ROOT, "include"), shim, "-o", obj], check=True)
        symbols = subprocess.run(["nm", "-g", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    java = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuNative.java")).read()
    for name in ("createNestedLoopPages", "destroyNestedLoopPages", "createNestedLoopBuild", "createNestedLoopJoin"):
        assert re.search(r"\bT Java_io_trino_gpu_GpuNative_%s\b" % name, symbols), name
        assert re.search(r"static native \w+ %s\(" % name, java), name
    planner = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuNestedLoopJoin.java")).read()
    assert "GpuNative.createNestedLoopJoin(" in planner and "RowExpressionSerializer.serialize(" in planner
    assert "GpuNestedLoopJoin.create(" in open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuOperatorFactories.java")).read()


def test_cpp_mirror_declares_the_classes():
    """include/presto_amd.hpp: the bridge and the two factories, and a translation unit that uses them compiles"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "mirror.cpp")
        with open(src, "w") as f:
            f.write('#include "presto_amd.hpp"\nusing namespace presto_amd;\n'
                    "std::vector<Page> run(NestedLoopJoinBridge& bridge, const std::vector<Page>& build, const std::vector<Page>& probe) {\n"
                    "    auto b = NestedLoopBuildOperatorFactory({PA_BIGINT}).createOperator(bridge);\n"
                    "    auto j = NestedLoopJoinOperatorFactory({PA_BIGINT}, {0}, {0}, call(PA_OP_LESS_THAN, PA_BOOLEAN, {field(1, PA_BIGINT), field(0, PA_BIGINT)}))"
                    ".createOperator(bridge);\n"
                    "    runDriver(build, {b.get()});\n    (void)bridge.rows();\n    return runDriver(probe, {j.get()});\n}\n")
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src], check=True)
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_nested_loop.cpp"))


# ---- the model, pinned by hand ----------------------------------------------------------------------------------------------------------
def test_model_plain_product_is_probe_major():
    probe = [(1, b"a"), (2, b"b"), (3, None)]
    build = [(10,), (20,)]
    assert NL.nested_loop(probe, build, [0, 1], [0]) == [(1, b"a", 10), (1, b"a", 20), (2, b"b", 10), (2, b"b", 20), (3, None, 10), (3, None, 20)]
    assert NL.nested_loop(probe, [], [0], [0]) == [] and NL.nested_loop([], build, [0], [0]) == []


def test_model_null_is_not_a_match():
    # p.x < b.y: the pair row is (b.y, p.x)
    f = lt(field(1, abi.BIGINT), field(0, abi.BIGINT))
    probe = [(1,), (None,), (5,)]
    build = [(3,), (None,), (6,)]
    assert NL.nested_loop(probe, build, [0], [0], f) == [(1, 3), (1, 6), (5, 6)]


def test_model_scalar_subquery_shape():
    f = call(abi.OP_GREATER_THAN, abi.BOOLEAN, field(1, abi.DOUBLE), field(0, abi.DOUBLE))
    assert NL.nested_loop([(1.5,), (2.5,), (float("nan"),), (3.0,)], [(2.5,)], [0], [], f) == [(3.0,)]


def test_model_errors_follow_every_pair():
    # p.x / b.y > 0 with one zero b.y: an error whatever else the product holds; behind a conjunct that is false for that pair, none
    div = call(abi.OP_GREATER_THAN, abi.BOOLEAN, call(abi.OP_DIVIDE, abi.BIGINT, field(1, abi.BIGINT), field(0, abi.BIGINT)), constant(0, abi.BIGINT))
    probe, build = [(4,), (8,)], [(2,), (0,), (1,)]
    assert NL.outcome(probe, build, [0], [0], div) == ("error", abi.ERR_DIVISION_BY_ZERO)
    guarded = and_(call(abi.OP_NOT_EQUAL, abi.BOOLEAN, field(0, abi.BIGINT), constant(0, abi.BIGINT)), div)
    assert NL.outcome(probe, build, [0], [0], guarded) == ("rows", [(4, 2), (4, 1), (8, 2), (8, 1)])
    assert M.evaluate(guarded, NL.pair_row((0,), (4,))) is False
