"""CPU-side checks of the streaming aggregation (pa_streaming_aggregation_create): exported, the ctypes mirror laid out as the header
lays it out, every invalid argument and every refusal of the contract reported at creation -- an invalid argument before a refusal,
both before the device is asked for --, no device -> a loud PA_ERR_NO_DEVICE, and the model the GPU tests compare against
(tests/streaming_agg_model.py) pinned by hand with the reference's known answers (TestStreamingAggregationOperator), restated as data."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import lib
from tests import agg_model as A
from tests import streaming_agg_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["input_channel_count", "input_types", "input_type_params", "group_by_count", "group_by_channels", "step", "aggregate_count", "aggregates",
          "output_mem", "stream"]
NAN = float("nan")
D122, D302 = abi.decimal(12, 2), abi.decimal(30, 2)
KEY_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, D122]
COUNT_STAR = (abi.AGG_COUNT_STAR, -1, None)


def has_gpu():
    return lib().pa_device_count() > 0


def accepted():
    """what a descriptor without a defect gives: an operator on a GPU, a loud refusal to run without one"""
    return abi.OK if has_gpu() else abi.ERR_NO_DEVICE


def create(input_types, group_by, aggregates, **kw):
    """the status of pa_streaming_aggregation_create; an operator that did come to be is closed again"""
    from presto_amd.operators import streaming_aggregation_desc
    d, keep = streaming_aggregation_desc(input_types, group_by, aggregates, **kw)
    h = C.c_void_p()
    rc = lib().pa_streaming_aggregation_create(C.byref(d), C.byref(h))
    if rc == abi.OK:
        lib().pa_op_close(h)
    return rc


def test_entry_point_is_exported():
    assert lib().pa_streaming_aggregation_create is not None
    from presto_amd.operators import StreamingAggregationOperator, StreamingAggregationOperatorFactory   # noqa: F401  (the Python mirrors)


def test_ctypes_layout_matches_the_header():
    """sizeof / offsetof of the descriptor, printed by a C program compiled against include/presto_amd.h."""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "presto_amd.h"\nint main(void) {\n')
            f.write('    printf("%d\\n", (int)sizeof(pa_streaming_aggregation_desc));\n')
            for name in FIELDS:
                f.write('    printf("%%d\\n", (int)offsetof(pa_streaming_aggregation_desc, %s));\n' % name)
            f.write("    return 0;\n}\n")
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    cls = abi.pa_streaming_aggregation_desc
    assert [name for name, _ in cls._fields_] == FIELDS
    assert got == [C.sizeof(cls)] + [getattr(cls, name).offset for name in FIELDS]


def test_invalid_arguments():
    from presto_amd.operators import streaming_aggregation_desc
    L = lib()
    h = C.c_void_p()
    types = [abi.BIGINT, abi.BIGINT, abi.BOOLEAN, abi.VARCHAR, abi.DATE]
    sum1 = (abi.AGG_SUM, 1, abi.BIGINT)
    assert L.pa_streaming_aggregation_create(None, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    d, keep = streaming_aggregation_desc(types, [0], [sum1])
    assert L.pa_streaming_aggregation_create(C.byref(d), None) == abi.ERR_INVALID_ARGUMENT
    # counts out of range
    for name, values in (("input_channel_count", (-1, 0)), ("group_by_count", (-1, 0, 9)), ("aggregate_count", (-1, 17))):
        for v in values:
            d, keep = streaming_aggregation_desc(types, [0], [sum1])
            setattr(d, name, v)
            assert L.pa_streaming_aggregation_create(C.byref(d), C.byref(h)) == abi.ERR_INVALID_ARGUMENT, (name, v)
    for name in ("input_types", "group_by_channels", "aggregates"):
        d, keep = streaming_aggregation_desc(types, [0], [sum1])
        setattr(d, name, None)
        assert L.pa_streaming_aggregation_create(C.byref(d), C.byref(h)) == abi.ERR_INVALID_ARGUMENT, name
    assert create(types, list(range(5)) + [0, 1, 2, 3], []) == abi.ERR_INVALID_ARGUMENT          # nine group channels
    assert create(types, [0], [COUNT_STAR] * 17) == abi.ERR_INVALID_ARGUMENT
    # channels out of range
    for channel in (-1, 5, 99):
        assert create(types, [channel], [sum1]) == abi.ERR_INVALID_ARGUMENT, channel
        assert create(types, [0], [(abi.AGG_SUM, channel, abi.BIGINT)]) == abi.ERR_INVALID_ARGUMENT, channel
        assert create(types, [0], [(abi.AGG_COUNT, channel, abi.BIGINT)]) == abi.ERR_INVALID_ARGUMENT, channel
    for mask in (-2, 5):
        assert create(types, [0], [(abi.AGG_SUM, 1, abi.BIGINT, mask)]) == abi.ERR_INVALID_ARGUMENT, mask
        assert create(types, [0], [(abi.AGG_COUNT_STAR, -1, None, mask)]) == abi.ERR_INVALID_ARGUMENT, mask
    # an unknown fn, step, type, output_mem
    for fn in (-1, 6, 99):
        assert create(types, [0], [(fn, 1, abi.BIGINT)]) == abi.ERR_INVALID_ARGUMENT, fn
    for step in (-1, 3):
        assert create(types, [0], [sum1], step=step) == abi.ERR_INVALID_ARGUMENT, step
    for bad in (-1, 10, 99):
        assert create(types + [bad], [0], [sum1]) == abi.ERR_INVALID_ARGUMENT, bad
    for mem in (-1, 2):
        assert create(types, [0], [sum1], output_mem=mem) == abi.ERR_INVALID_ARGUMENT, mem
    # a mask that is not BOOLEAN, an input_type that differs from the channel's
    assert create(types, [0], [(abi.AGG_SUM, 1, abi.BIGINT, 0)]) == abi.ERR_INVALID_ARGUMENT
    assert create(types, [0], [(abi.AGG_COUNT_STAR, -1, None, 3)]) == abi.ERR_INVALID_ARGUMENT
    assert create(types, [0], [(abi.AGG_SUM, 1, abi.INTEGER)]) == abi.ERR_INVALID_ARGUMENT
    assert create(types, [0], [(abi.AGG_MIN, 4, abi.INTEGER)]) == abi.ERR_INVALID_ARGUMENT      # DATE is not INTEGER
    # sum / avg over VARCHAR, BOOLEAN or DATE
    for fn in (abi.AGG_SUM, abi.AGG_AVG):
        for channel in (2, 3, 4):
            assert create(types, [0], [(fn, channel, types[channel])]) == abi.ERR_INVALID_ARGUMENT, (fn, channel)


def test_refusals():
    types = [abi.BIGINT, abi.DOUBLE, D122, D302, abi.VARCHAR, abi.ROW, abi.BOOLEAN]
    params = [0, 0, abi.type_param(D122), abi.type_param(D302), 0, 0, 0]
    ok = (abi.AGG_SUM, 1, abi.DOUBLE)
    for step in (abi.STEP_PARTIAL, abi.STEP_FINAL):
        assert create(types, [0], [ok], step=step, type_params=params) == abi.ERR_NOT_SUPPORTED, step
    for channel in (3, 5):      # PA_LONG_DECIMAL / PA_ROW group channels
        assert create(types, [0, channel], [ok], type_params=params) == abi.ERR_NOT_SUPPORTED, channel
    for fn in (abi.AGG_SUM, abi.AGG_AVG):
        for channel in (2, 3):
            assert create(types, [0], [(fn, channel, int(types[channel]))], type_params=params) == abi.ERR_NOT_SUPPORTED, (fn, channel)
    for fn in (abi.AGG_MIN, abi.AGG_MAX):
        for channel in (3, 4, 5):
            assert create(types, [0], [(fn, channel, int(types[channel]))], type_params=params) == abi.ERR_NOT_SUPPORTED, (fn, channel)
    assert create(types, [0], [(abi.AGG_COUNT, 5, abi.ROW)], type_params=params) == abi.ERR_NOT_SUPPORTED
    assert create([abi.BIGINT] * 65, [0], [COUNT_STAR]) == abi.ERR_NOT_SUPPORTED


def test_an_invalid_argument_is_reported_before_a_refusal():
    types = [abi.BIGINT, abi.DOUBLE, D122, D302, abi.VARCHAR, abi.ROW, abi.BOOLEAN]
    refused = (abi.AGG_MIN, 4, abi.VARCHAR)
    assert create(types, [0], [refused]) == abi.ERR_NOT_SUPPORTED
    assert create(types, [0], [refused, (abi.AGG_SUM, 9, abi.BIGINT)]) == abi.ERR_INVALID_ARGUMENT
    assert create(types, [0], [refused, (abi.AGG_SUM, 4, abi.VARCHAR)]) == abi.ERR_INVALID_ARGUMENT
    assert create(types, [0], [refused], output_mem=7) == abi.ERR_INVALID_ARGUMENT
    assert create(types, [5], [(abi.AGG_SUM, 1, abi.DOUBLE, 0)]) == abi.ERR_INVALID_ARGUMENT       # ROW key, but the mask is not BOOLEAN
    assert create(types, [5, 9], []) == abi.ERR_INVALID_ARGUMENT                                     # ROW key, but a channel out of range
    assert create(types, [0], [(abi.AGG_SUM, 1, abi.DOUBLE)], step=abi.STEP_PARTIAL, output_mem=-1) == abi.ERR_INVALID_ARGUMENT
    assert create(types, [0], [(7, 1, abi.DOUBLE)], step=abi.STEP_FINAL) == abi.ERR_INVALID_ARGUMENT
    assert create([abi.BIGINT] * 65 + [99], [0], []) == abi.ERR_INVALID_ARGUMENT


def test_what_the_contract_takes():
    """every key type; every aggregate over every type the contract lists; no aggregate at all: nothing but the device is missing"""
    params = [abi.type_param(t) if isinstance(t, abi.DecimalType) else 0 for t in KEY_TYPES]
    assert create(KEY_TYPES, list(range(8)), [], type_params=params) == accepted()
    types = [abi.BIGINT, abi.INTEGER, abi.DOUBLE, abi.REAL, abi.DATE, abi.BOOLEAN, D122, abi.VARCHAR, abi.ROW]
    params = [abi.type_param(t) if isinstance(t, abi.DecimalType) else 0 for t in types]
    aggs = [COUNT_STAR, (abi.AGG_COUNT_STAR, -1, None, 5)]
    aggs += [(abi.AGG_COUNT, c, int(types[c])) for c in range(8)]
    assert create(types, [7], aggs, type_params=params) == accepted()
    aggs = [(fn, c, int(types[c]), 5) for fn in (abi.AGG_SUM, abi.AGG_AVG) for c in range(4)]
    assert create(types, [0], aggs, type_params=params) == accepted()
    aggs = [(fn, c, int(types[c])) for fn in (abi.AGG_MIN, abi.AGG_MAX) for c in range(7)]
    assert create(types, [0, 1], aggs, type_params=params, output_mem=abi.MEM_DEVICE) == accepted()


@pytest.mark.skipif(has_gpu(), reason="container without a GPU only")
def test_no_device_fails_loudly():
    assert create([abi.BIGINT, abi.BIGINT], [0], [(abi.AGG_SUM, 1, abi.BIGINT)]) == abi.ERR_NO_DEVICE
    assert b"no" in lib().pa_last_error().lower()


def test_sources_and_build_list():
    makefile = open(os.path.join(ROOT, "presto_amd", "csrc", "Makefile")).read()
    assert "op_streaming_agg.cpp" in makefile and "streaming_agg_kernels.hip" in makefile
    kernels = open(os.path.join(ROOT, "presto_amd", "csrc", "streaming_agg_kernels.hpp")).read()
    assert re.search(r"kStreamAggTile\s*=\s*1024", kernels) and "launch_stream_agg_reduce(" in kernels


def test_jni_shim_and_java_natives():
    """jni/presto_amd_jni.c compiles against the stand-in jni.h and exports the native GpuNative.java declares"""
    shim = os.path.join(ROOT, "jni", "presto_amd_jni.c")
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "shim.o")
        subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-fPIC", "-I" + os.path.join(ROOT, "jni", "stub"), "-I" + os.path.join(ROOT, "include"), shim, "-o", obj], check=True)
        symbols = subprocess.run(["nm", "-g", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    java = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuNative.java")).read()
    assert re.search(r"\bT Java_io_trino_gpu_GpuNative_createStreamingAggregation\b", symbols)
    assert re.search(r"static native long createStreamingAggregation\(", java)
    planner = open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuStreamingAggregation.java")).read()
    assert "GpuNative.createStreamingAggregation(" in planner
    assert "GpuStreamingAggregation.create(" in open(os.path.join(ROOT, "java", "io", "trino", "gpu", "GpuOperatorFactories.java")).read()


def test_cpp_mirror_declares_the_factory():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "mirror.cpp")
        with open(src, "w") as f:
            f.write('#include "presto_amd.hpp"\nusing namespace presto_amd;\n'
                    "std::vector<Page> run(const std::vector<Page>& pages) {\n"
                    "    auto op = createStreamingAggregationOperator({PA_BIGINT, PA_DOUBLE, PA_BOOLEAN}, {0},\n"
                    "                                                 {{PA_AGG_COUNT_STAR, -1, -1, 0}, {PA_AGG_AVG, 1, 2, PA_DOUBLE}});\n"
                    "    return runDriver(pages, {op.get()});\n}\n")
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src], check=True)


# ---- the reference's known answers (TestStreamingAggregationOperator), as data --------------------------------------------------------------
# (types, group channels, aggregates, input pages as lists of rows, expected rows); addSequencePage(n, 0, k, v): BOOLEAN i % 2 == 0,
# the key k + i (a VARCHAR key as its decimal string), BIGINT v + i
def _sequence(n, key, value, varchar):
    return [(i % 2 == 0, str(key + i).encode() if varchar else float(key + i), value + i) for i in range(n)]


VARCHAR_SETUP = ([abi.BOOLEAN, abi.VARCHAR, abi.BIGINT], [1], [(abi.AGG_COUNT, 0, abi.BOOLEAN), (abi.AGG_SUM, 2, abi.BIGINT)])
KATS = {
    "test": ([abi.BOOLEAN, abi.DOUBLE, abi.BIGINT], [1], [(abi.AGG_COUNT, 0, abi.BOOLEAN), (abi.AGG_SUM, 2, abi.BIGINT)],
             [_sequence(3, 0, 1, False) + [(True, 3.0, 4), (False, 3.0, 5)],
              [(True, 3.0, 6), (False, 4.0, 7), (True, 4.0, 8), (False, 4.0, 9), (True, 4.0, 10)],
              [(False, 5.0, 11), (True, 5.0, 12), (False, 5.0, 13), (True, 5.0, 14), (False, 5.0, 15)],
              _sequence(3, 6, 16, False) + [(False, NAN, 1), (False, NAN, 10), (False, None, 2), (False, None, 20)]],
             [(0.0, 1, 1), (1.0, 1, 2), (2.0, 1, 3), (3.0, 3, 15), (4.0, 4, 34), (5.0, 5, 65), (6.0, 1, 16), (7.0, 1, 17), (8.0, 1, 18), (NAN, 2, 11),
              (None, 2, 22)]),
    "testSinglePage": VARCHAR_SETUP + ([[(False, b"a", 5)]], [(b"a", 1, 5)]),
    "testSingleGroupingValue": VARCHAR_SETUP + (
        [[(True, b"a", 1), (False, b"a", 2), (True, b"a", 3), (False, b"a", 4), (True, b"a", 5)], [(False, b"a", 6), (True, b"a", 7), (False, b"a", 8)], [], [],
         [(True, b"a", 9), (False, b"a", 10)]],
        [(b"a", 10, 55)]),
    "testUniqueGroupingValues": VARCHAR_SETUP + ([_sequence(10, 0, 0, True), _sequence(10, 10, 10, True)], [(str(i).encode(), 1, i) for i in range(20)]),
    "testEmptyInput": VARCHAR_SETUP + ([], []),
}


def same_rows(types, got, want):
    """rows compared value by value: floats by bit pattern with every NaN one value (agg_model.bits)"""
    return [tuple(A.bits(t, v) for t, v in zip(types, r)) for r in got] == [tuple(A.bits(t, v) for t, v in zip(types, r)) for r in want]


@pytest.mark.parametrize("name", sorted(KATS))
def test_model_gives_the_references_known_answers(name):
    types, group, aggs, pages, want = KATS[name]
    rows = [r for p in pages for r in p]
    got, error = S.expected_rows(rows, types, group, aggs)
    assert error is None
    out_types = [types[c] for c in group] + [A.result_type(a[0], a[2]) for a in aggs]
    assert len(want) == (11 if name == "test" else len(want))
    assert same_rows(out_types, got, want), (got, want)


def test_model_runs_and_first_row_keys():
    types = [abi.DOUBLE, abi.VARCHAR, abi.BIGINT]
    rows = [(0.0, b"", 1), (-0.0, b"", 2), (NAN, b"", 3), (A.NAN_PAYLOAD, b"", 4), (NAN, b"x", 5), (None, b"x", 6), (None, b"x", 7), (None, None, 8),
            (1.0, None, 9), (1.0, None, 10), (0.0, b"", 11)]
    runs = S.runs(rows, types, [0, 1])
    assert [[r[2] for r in members] for _, members in runs] == [[1, 2], [3, 4], [5], [6, 7], [8], [9, 10], [11]]
    # the key is the first row's: +0.0, not the -0.0 that follows it; the first NaN's payload
    assert A.bits(abi.DOUBLE, runs[0][0][0]) == A.bits(abi.DOUBLE, 0.0) and runs[1][0][0] != runs[1][0][0]
    # equal keys that are not adjacent are two runs
    assert S.not_distinct([abi.DOUBLE, abi.VARCHAR], rows[0][:2], rows[10][:2])


def test_model_masks_nulls_and_empty_runs():
    types = [abi.BIGINT, abi.BIGINT, abi.BOOLEAN]
    rows = [(1, 5, True), (1, None, True), (1, 7, None), (1, 9, False), (2, None, True), (2, 4, False), (3, 1, True)]
    aggs = [(abi.AGG_COUNT_STAR, -1, None, 2), (abi.AGG_COUNT, 1, abi.BIGINT, 2), (abi.AGG_SUM, 1, abi.BIGINT, 2), (abi.AGG_MIN, 1, abi.BIGINT), COUNT_STAR]
    got, error = S.expected_rows(rows, types, [0], aggs)
    assert error is None and got == [(1, 2, 1, 5, 5, 4), (2, 1, 0, None, 4, 2), (3, 1, 1, 1, 1, 1)]


def test_model_sum_is_add_exact_in_row_order():
    big = 2 ** 63 - 1
    types = [abi.BIGINT, abi.BIGINT]
    aggs = [(abi.AGG_SUM, 1, abi.BIGINT)]
    # a prefix that leaves int64 and comes back: an error, whatever the neighbours hold
    got, error = S.expected_rows([(1, 3), (2, big), (2, 1), (2, -5), (3, 4)], types, [0], aggs)
    assert got == [(1, 3)] and error == ("error", abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE)
    # the same values in an order whose prefixes fit
    got, error = S.expected_rows([(1, 3), (2, big), (2, -5), (2, 1), (3, 4)], types, [0], aggs)
    assert error is None and got == [(1, 3), (2, big - 4), (3, 4)]
    # two runs that would overflow as one
    got, error = S.expected_rows([(1, big), (2, big)], types, [0], aggs)
    assert error is None and got == [(1, big), (2, big)]
    # INTEGER: the int64 total, then the column's range
    got, error = S.expected_rows([(1, 2 ** 31 - 1), (1, 1), (1, -1)], [abi.BIGINT, abi.INTEGER], [0], [(abi.AGG_SUM, 1, abi.INTEGER)])
    assert error is None and got == [(1, 2 ** 31 - 1)]
    got, error = S.expected_rows([(1, 2 ** 31 - 1), (1, 1)], [abi.BIGINT, abi.INTEGER], [0], [(abi.AGG_SUM, 1, abi.INTEGER)])
    assert error == ("error", abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE)


def test_model_floating_results():
    types = [abi.BIGINT, abi.DOUBLE, abi.REAL]
    rows = [(1, -0.0, np.float32(1.5)), (1, -0.0, np.float32(2.5)), (2, NAN, np.float32(-0.0)), (2, 1.0, np.float32(0.0))]
    aggs = [(abi.AGG_SUM, 1, abi.DOUBLE), (abi.AGG_AVG, 2, abi.REAL), (abi.AGG_MIN, 1, abi.DOUBLE), (abi.AGG_MAX, 1, abi.DOUBLE), (abi.AGG_MIN, 2, abi.REAL),
            (abi.AGG_MAX, 2, abi.REAL)]
    got, error = S.expected_rows(rows, types, [0], aggs)
    out_types = [abi.BIGINT, abi.DOUBLE, abi.REAL, abi.DOUBLE, abi.DOUBLE, abi.REAL, abi.REAL]
    # the sum starts at +0.0; max is in Double.compare order: NaN above everything, +0.0 above -0.0
    want = [(1, 0.0, np.float32(2.0), -0.0, -0.0, np.float32(1.5), np.float32(2.5)), (2, NAN, np.float32(0.0), 1.0, NAN, np.float32(-0.0), np.float32(0.0))]
    assert error is None and same_rows(out_types, got, want), got
